"""Raw blobs for the nested bincode tests (tests/test_nested_bincode_ref.py,
tests/test_gpu_nested_bincode.py): a field-by-field writer that takes plain
lists as they stand — unsorted, duplicated, zero, with any length word — so
every malformed kind and every capacity + 1 can be spelled out. Needs no GPU.

Specs (lists of pairs, nothing is sorted or checked):
  clock    [(actor, counter), ...]
  deferred [(clock, [element, ...]), ...]
  orswot   (clock, [(member, clock), ...], deferred)
  mvreg    [(clock, val), ...]
  map      (clock, [(key, entry clock, value), ...], deferred), value an orswot
           spec (kind "orswot") or a map spec of mvreg values (kind "nested")
"""
from __future__ import annotations

import copy
import struct

ENONCANON, ECAPACITY = "ENONCANON", "ECAPACITY"


class Raw:
    """widths: (actor, key, member) for kind "orswot", (actor, key, inner key, val) for "nested"."""

    def __init__(self, kind, widths):
        self.kind, self.w = kind, tuple(widths)
        self.b = bytearray()
        self.lens = []  # (position, label) of every length word

    def L(self, n, label):
        self.lens.append((len(self.b), label))
        self.b += struct.pack("<Q", n)

    def u(self, v, w):
        self.b += int(v).to_bytes(w, "little")

    def clock(self, pairs, label):
        self.L(len(pairs), label)
        for a, c in pairs:
            self.u(a, self.w[0])
            self.u(c, 8)

    def deferred(self, defs, we, label):
        self.L(len(defs), label + " n")
        for c, xs in defs:
            self.clock(c, label + " clock")
            self.L(len(xs), label + " set")
            for x in xs:
                self.u(x, we)

    def orswot(self, o):
        clock, members, defs = o
        self.clock(clock, "orswot clock")
        self.L(len(members), "members")
        for m, c in members:
            self.u(m, self.w[2])
            self.clock(c, "member clock")
        self.deferred(defs, self.w[2], "orswot deferred")

    def mvreg(self, vals):
        self.L(len(vals), "values")
        for c, v in vals:
            self.clock(c, "value clock")
            self.u(v, self.w[3])

    def map(self, m, depth=0):
        clock, entries, defs = m
        inner = self.kind == "nested" and depth == 1
        pre = "inner " if inner else ""
        wk = self.w[2] if inner else self.w[1]
        self.clock(clock, pre + "map clock")
        self.L(len(entries), pre + "entries")
        for key, ec, v in entries:
            self.u(key, wk)
            self.clock(ec, pre + "entry clock")
            if self.kind == "orswot":
                self.orswot(v)
            elif inner:
                self.mvreg(v)
            else:
                self.map(v, 1)
        self.deferred(defs, wk, pre + "deferred")
        return self


def raw(kind, widths, spec):
    """-> (blob, [(position, label) of every length word])"""
    r = Raw(kind, widths).map(spec)
    return bytes(r.b), r.lens


WIDTHS = {"orswot": (1, 1, 1), "nested": (1, 1, 1, 1)}

# the well-formed blobs every malformed one is a change of (n_actors >= 3)
GOOD = {
    "orswot": ([(0, 3), (1, 2)],
               [(5, [(0, 3)], ([(0, 3), (1, 1)], [(9, [(0, 3), (1, 1)]), (4, [(0, 1)])],
                               [([(2, 2)], [8, 7]), ([(2, 1)], [7])])),
                (8, [(1, 2)], ([(1, 2)], [(1, [(1, 2)])], []))],
               [([(0, 4), (1, 1)], [5, 6]), ([(0, 4)], [5])]),
    "nested": ([(0, 3), (1, 2)],
               [(5, [(0, 3)], ([(0, 3), (1, 1)],
                               [(4, [(0, 1)], [([(0, 1)], 40)]), (9, [(0, 3), (1, 1)], [([(0, 3)], 90), ([(1, 1)], 91)])],
                               [([(2, 2)], [7, 8]), ([(2, 1)], [7])])),
                (8, [(1, 2)], ([(1, 2)], [(1, [(1, 2)], [])], []))],
               [([(0, 4), (1, 1)], [5, 6]), ([(0, 4)], [5])]),
}


def _edit(kind, f):
    s = copy.deepcopy(GOOD[kind])
    s = f(s) or s
    return raw(kind, WIDTHS[kind], s)[0]


def malformed(kind, n_actors):
    """name -> (blob, why): every CRDT_ENONCANON kind at outer and at nested
    depth. why: a regex of the restatement's FormatError, or None where only
    the GPU can tell (an actor >= n_actors)."""
    A = n_actors
    good, lens = raw(kind, WIDTHS[kind], GOOD[kind])
    out = {}

    def put(name, f, why):
        out[name] = (_edit(kind, f), why)

    # --- at outer depth
    put("zero_counter_map_clock", lambda s: s[0].__setitem__(0, (0, 0)), "zero counter")
    put("actor_past_n_actors_map_clock", lambda s: s[0].__setitem__(1, (A, 2)), None)
    put("actors_descending_map_clock", lambda s: s[0].reverse(), "actors not strictly")
    put("actors_equal_entry_clock", lambda s: s[1][0][1].append((0, 3)), "actors not strictly")
    put("keys_descending", lambda s: s[1].reverse(), "^keys not strictly")
    put("keys_equal", lambda s: s[1].__setitem__(1, (5,) + s[1][1][1:]), "^keys not strictly")
    put("deferred_keys_descending", lambda s: s[2][0][1].reverse(), "deferred-set keys")
    put("deferred_keys_equal", lambda s: s[2][0][1].__setitem__(1, 5), "deferred-set keys")
    put("duplicate_deferred_clock", lambda s: s[2].__setitem__(1, (s[2][0][0], [5])), "duplicate deferred clock")
    put("zero_counter_deferred_clock", lambda s: s[2][1][0].__setitem__(0, (0, 0)), "zero counter")
    # --- at nested depth
    v = lambda s: s[1][0][2]  # noqa: E731  the first entry's value
    put("zero_counter_value_clock", lambda s: v(s)[0].__setitem__(1, (1, 0)), "zero counter")
    put("actor_past_n_actors_value_clock", lambda s: v(s)[0].__setitem__(1, (A + 1, 1)), None)
    put("actors_descending_value_clock", lambda s: v(s)[0].reverse(), "actors not strictly")
    put("duplicate_nested_deferred_clock", lambda s: v(s)[2].__setitem__(1, (v(s)[2][0][0], [7])),
        "duplicate deferred clock")
    put("zero_counter_nested_deferred_clock", lambda s: v(s)[2][0][0].__setitem__(0, (2, 0)), "zero counter")
    if kind == "orswot":
        put("duplicate_member", lambda s: v(s)[1].__setitem__(1, (9, [(0, 1)])), "duplicate member")
        put("duplicate_deferred_set_member", lambda s: v(s)[2][0][1].__setitem__(1, 8), "duplicate deferred-set member")
        put("zero_counter_member_clock", lambda s: v(s)[1][0][1].__setitem__(0, (0, 0)), "zero counter")
        put("actors_equal_member_clock", lambda s: v(s)[1][0][1].__setitem__(1, (0, 9)), "actors not strictly")
    else:
        put("inner_keys_descending", lambda s: v(s)[1].reverse(), "^keys not strictly")
        put("inner_deferred_keys_descending", lambda s: v(s)[2][0][1].reverse(), "deferred-set keys")
        put("zero_counter_register_clock", lambda s: v(s)[1][1][2].__setitem__(0, ([(0, 0)], 90)), "zero counter")
        put("actors_equal_inner_entry_clock", lambda s: v(s)[1][1][1].__setitem__(1, (0, 9)), "actors not strictly")
    # --- the bytes themselves
    out["one_byte_short"] = (good[:-1], "truncated|length word")
    out["ends_inside_the_first_value"] = (good[:lens[6][0] + 3], "truncated|length word")
    out["one_byte_extra"] = (good + b"\0", "trailing")
    seen = set()
    for pos, label in lens:  # a 2^63 length word at each of the length positions
        if label in seen:
            continue
        seen.add(label)
        out["length_2_63 " + label] = (good[:pos] + struct.pack("<Q", 1 << 63) + good[pos + 8:], "length word")
    return out


LENGTH_LABELS = {
    "orswot": {"map clock", "entries", "entry clock", "orswot clock", "members", "member clock", "orswot deferred n",
               "orswot deferred clock", "orswot deferred set", "deferred n", "deferred clock", "deferred set"},
    "nested": {"map clock", "entries", "entry clock", "inner map clock", "inner entries", "inner entry clock",
               "values", "value clock", "inner deferred n", "inner deferred clock", "inner deferred set", "deferred n",
               "deferred clock", "deferred set"},
}


def _clk(j):
    return [(0, j + 1)]


def over_capacity(kind, caps):
    """name -> blob: well-formed, one count at its capacity + 1. caps: the
    orswot slab's dict, or ((kcap, dcap, scap), (kcap, mcap, dcap, scap))."""
    w = WIDTHS[kind]
    out = {}
    if kind == "orswot":
        c = caps
        o = lambda members=(), defs=(): ([], list(members), list(defs))  # noqa: E731
        out["kcap"] = ([], [(k, [], o()) for k in range(c["kcap"] + 1)], [])
        out["mcap"] = ([], [(1, [], o(members=[(m, []) for m in range(c["mcap"] + 1)]))], [])
        out["vdcap"] = ([], [(1, [], o(defs=[(_clk(j), [1]) for j in range(c["vdcap"] + 1)]))], [])
        out["vscap"] = ([], [(1, [], o(defs=[(_clk(0), list(range(c["vscap"] + 1)))]))], [])
        out["dcap"] = ([], [], [(_clk(j), [1]) for j in range(c["dcap"] + 1)])
        out["scap"] = ([], [], [(_clk(0), list(range(c["scap"] + 1)))])
    else:
        (kcap, dcap, scap), (ik, im, idc, isc) = caps
        i = lambda entries=(), defs=(): ([], list(entries), list(defs))  # noqa: E731
        out["kcap"] = ([], [(k, [], i()) for k in range(kcap + 1)], [])
        out["dcap"] = ([], [], [(_clk(j), [1]) for j in range(dcap + 1)])
        out["scap"] = ([], [], [(_clk(0), list(range(scap + 1)))])
        out["inner kcap"] = ([], [(1, [], i(entries=[(k, [], []) for k in range(ik + 1)]))], [])
        out["inner mcap"] = ([], [(1, [], i(entries=[(2, [], [(_clk(j), j) for j in range(im + 1)])]))], [])
        out["inner dcap"] = ([], [(1, [], i(defs=[(_clk(j), [1]) for j in range(idc + 1)]))], [])
        out["inner scap"] = ([], [(1, [], i(defs=[(_clk(0), list(range(isc + 1)))]))], [])
    return {k: raw(kind, w, s)[0] for k, s in out.items()}
