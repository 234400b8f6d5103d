"""Inputs shared by the LWWReg tests (host and GPU): seeded registers and op
lists over small alphabets, so that equal markers, and with them conflicts
and equal-marker no-ops, are frequent; and the closed form of an op list,
written out in Python."""
import random

MARKERS_1 = (0, 1, 1 << 32, (1 << 64) - 1)  # 4 one-word markers, the u64 edges among them
# 4 two-word markers: two differ only in word 1, and word 0 decides against word 1 ((1, 9) < (2, 0))
MARKERS_2 = ((1, 9), (2, 0), (2, (1 << 64) - 1), ((1 << 64) - 1, 0))
VALS = (7, 8, (1 << 64) - 1)


def markers(marker_words):
    return MARKERS_1 if marker_words == 1 else MARKERS_2


def rnd_reg(rng, marker_words):
    return (rng.choice(VALS), rng.choice(markers(marker_words)))


def rnd_lists(seed, n, marker_words, max_len=6):
    """n (start register, op list) pairs."""
    rng = random.Random(seed)
    return [(rnd_reg(rng, marker_words), [rnd_reg(rng, marker_words) for _ in range(rng.randrange(0, max_len + 1))])
            for _ in range(n)]


def closed_form(reg, ops):
    """The final state and every op's Result without applying anything in
    order: the state op i meets is the FIRST element of o_0..o_{i-1} attaining
    their largest marker (o_0 = reg); op i errs iff its marker equals that
    marker and its value differs; the final state is the first element of
    o_0..o_k attaining the largest marker. -> (reg, [err per op])."""
    seq = [reg] + list(ops)

    def first_max(k):  # over seq[0..k)
        top = max(m for _, m in seq[:k])
        return next(r for r in seq[:k] if r[1] == top)

    errs = []
    for i in range(1, len(seq)):
        val, marker = first_max(i)
        errs.append(seq[i][1] == marker and seq[i][0] != val)
    return first_max(len(seq)), errs
