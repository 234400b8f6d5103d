/*
 * crdts_hip.h — C ABI of the MI355X batched CRDT merge engine.
 *
 * This is the drop-in boundary for ONE path of etsangsplk/rust-crdt (crate
 * `crdts` 1.3.0): the state-based join
 *
 *     pub trait CvRDT { fn merge(&mut self, other: &Self); }   // src/traits.rs:9-12
 *
 * for VClock (src/vclock.rs:131-137), GCounter (src/gcounter.rs:58-62),
 * PNCounter (src/pncounter.rs:90-95) and Orswot incl. deferred removes
 * (src/orswot.rs:87-157, 195-211, 235-243). The reference merges ONE pair per
 * call; every entry point here merges a BATCH of independent pairs
 * (self[i] ⊔= other[i]) on one MI355X, with per-object results bit-exact with
 * calling the reference `merge` on each pair.
 *
 * Conventions
 *  - Plain pointers and sizes only. Pointers named `d_*` are DEVICE pointers
 *    (hipMalloc'd or torch tensors' data_ptr), `h_*` are host pointers.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - Return 0 on success, a negative CRDT_E* code otherwise. Nothing aborts.
 *    Launches are asynchronous: argument errors are returned immediately,
 *    record-level errors found by a kernel (non-canonical / oversized input)
 *    are latched in the context and returned by crdt_ctx_status().
 *  - The caller owns every buffer. A crdt_ctx owns only a small device status
 *    word; distinct contexts may be used from distinct threads concurrently.
 *  - Orientation is fixed and matters (Orswot merge is structurally
 *    non-commutative, src/orswot.rs:98-103 vs :132-137):
 *    output = self.merge(&other), exactly.
 *
 * Actors are interned by the caller to dense u32 ids in the same order as the
 * reference's `Ord` on actors (BTreeMap order, src/vclock.rs:54-57); members
 * are interned to u64 keys bijectively (the caller's intern table).
 */
#ifndef CRDTS_HIP_H
#define CRDTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRDT_ABI_VERSION 1

#define CRDT_OK 0
#define CRDT_EINVAL (-1)     /* bad argument (null pointer, zero actors, misaligned) */
#define CRDT_ENONCANON (-2)  /* an input record is not canonical / inconsistent     */
#define CRDT_EHIP (-3)       /* HIP runtime error                                  */
#define CRDT_ECAPACITY (-4)  /* output capacity too small                          */
#define CRDT_ECOMM (-5)      /* RCCL / communicator error                          */
#define CRDT_ENODEV (-6)     /* no usable gfx950 device                            */

typedef struct crdt_ctx crdt_ctx;

/* Context: binds a device and owns a device-side status word. */
int crdt_ctx_create(crdt_ctx** out, int device);
int crdt_ctx_destroy(crdt_ctx* ctx);
/* Synchronizes `stream`, returns the first record-level error latched by any
 * kernel launched through ctx since the last call (and clears it). */
int crdt_ctx_status(crdt_ctx* ctx, void* stream);
const char* crdt_strerror(int code);
int crdt_abi_version(void);
/* Capacity (<= 65536, the default) of the context's list of objects handed
 * from the fast Orswot / apply kernels to their general kernels (an Orswot
 * merge splits it in two halves: the general kernel's objects and the big
 * objects the join hands straight to the block-per-object kernel). Past a
 * list's capacity the kernels scan every output offset instead; results are
 * identical. Lowering it exercises that overflow path (tests). */
int crdt_ctx_set_list_cap(crdt_ctx* ctx, uint32_t cap);
/* Host synchronisations with the device (stream waits) the context's replica
 * joins have made so far (crdt_orswot_replica_join*: 3 per call in the steady
 * state). A counter for callers that profile the join's per-step cost. */
uint64_t crdt_ctx_host_syncs(const crdt_ctx* ctx);
/* Largest device arena (bytes) the context may allocate for the replica
 * exchanges (crdt_orswot_replica_join*, crdt_replica_*_max_transport);
 * 0 (the default) = no limit. A call whose arena would exceed it returns
 * CRDT_ECAPACITY on every rank of the exchange (the verdict is all-gathered
 * before any data moves), and the context keeps the arena it had. */
int crdt_ctx_set_arena_limit(crdt_ctx* ctx, size_t max_bytes);

/* ------------------------------------------------------------------------ *
 * Dense clocks and counters.
 *
 * Layout: row-major u64[n_obj][n_actors]; row i is one VClock / GCounter, slot
 * a holds the counter of interned actor a, 0 = absent (canonical: the
 * reference never stores a 0, `witness` src/vclock.rs:159-163).
 *
 * self[i] := pointwise max(self[i], other[i]), in place.
 *   VClock::merge   src/vclock.rs:131-137   (witness loop == pointwise max)
 *   GCounter::merge src/gcounter.rs:58-62   (delegates to VClock::merge)
 *   PNCounter::merge src/pncounter.rs:90-95 (P and N rows: pass the [P|N]
 *                    row of 2*n_actors slots, see crdt_pncounter_merge)
 * ------------------------------------------------------------------------ */
int crdt_vclock_dense_merge(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other,
                            size_t n_obj, uint32_t n_actors, void* stream);
int crdt_gcounter_merge(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other,
                        size_t n_obj, uint32_t n_actors, void* stream);
/* PNCounter row = P slots [0, n_actors) then N slots [n_actors, 2*n_actors). */
int crdt_pncounter_merge(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other,
                         size_t n_obj, uint32_t n_actors, void* stream);

/* The same with HOST rows (H2D, merge, D2H, synchronous): the PCIe-inclusive
 * path of a host `merge_batch(&mut [T], &[T])` for VClock / GCounter
 * (n_slots = n_actors) and PNCounter (n_slots = 2 * n_actors, [P|N] rows). */
int crdt_dense_merge_host(crdt_ctx* ctx, uint64_t* h_self, const uint64_t* h_other, size_t n_obj,
                          uint32_t n_slots);

/* ------------------------------------------------------------------------ *
 * Sparse (CSR) clocks and counters, for actor universes too large for dense
 * rows (a 1024-actor universe with ~48 actors per
 * clock is 8 KB dense and ~0.6 KB here). The reference clock is a
 * BTreeMap<A, u64> (src/vclock.rs:54-57): here object i's clock is the run
 * of entries [off[i], off[i] + len[i]) of act / ctr — actors strictly
 * increasing (BTreeMap order of the interned ids), counters > 0 (`witness`
 * never stores 0, :159-163). A batch may have gaps between runs.
 *
 * out[i] := self[i].merge(&other[i]): the sorted union of the two runs with
 * the larger counter per actor — VClock::merge src/vclock.rs:131-137;
 * GCounter::merge src/gcounter.rs:58-62; PNCounter::merge
 * src/pncounter.rs:90-95 (its P and N clocks are two batches). The call
 * writes out.off[i] := self.off[i] + other.off[i] and out.len[i] := the
 * union's length (<= self.len[i] + other.len[i]), and the entries there, so
 * out.n_entries >= self.n_entries + other.n_entries suffices and the output
 * is itself a valid (gapped) input batch.
 * PRECONDITION (checked on the device; a violation latches CRDT_EINVAL and
 * the object's out.len is 0): on each side runs lie inside [0, n_entries)
 * at increasing, non-overlapping offsets (off[i] + len[i] <= off[i+1]). A
 * run that is not canonical (actors not strictly increasing, a zero counter)
 * latches CRDT_ENONCANON (out.len 0). Runs of any length (<= 64 entries per
 * side take the loop-free path).
 * ------------------------------------------------------------------------ */
typedef struct crdt_clock_csr {
  const uint64_t* off;   /* device, n_obj: first entry of object i's run */
  const uint32_t* len;   /* device, n_obj: entries of the run            */
  const uint32_t* act;   /* device, n_entries: interned actor ids          */
  const uint64_t* ctr;   /* device, n_entries: counters                    */
  size_t n_obj;
  size_t n_entries;      /* extent of act / ctr (bounds checks)            */
} crdt_clock_csr;
typedef struct crdt_clock_csr_out {
  uint64_t* off;         /* device, n_obj (written)                        */
  uint32_t* len;         /* device, n_obj (written)                        */
  uint32_t* act;         /* device, n_entries                              */
  uint64_t* ctr;         /* device, n_entries                              */
  size_t n_entries;
} crdt_clock_csr_out;
int crdt_vclock_csr_merge(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                          const crdt_clock_csr_out* out, void* stream);
int crdt_gcounter_csr_merge(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                            const crdt_clock_csr_out* out, void* stream);
/* PNCounter: its P and N clocks as two batches of the same n_obj (one call). */
int crdt_pncounter_csr_merge(crdt_ctx* ctx, const crdt_clock_csr* self_p, const crdt_clock_csr* self_n,
                             const crdt_clock_csr* other_p, const crdt_clock_csr* other_n,
                             const crdt_clock_csr_out* out_p, const crdt_clock_csr_out* out_n, void* stream);

/* ------------------------------------------------------------------------ *
 * Clock and counter fold (clock_fold.hip): out[i] = reps[0][i].merge(reps[1][i])
 * .merge(reps[2][i])... of VClock::merge (src/vclock.rs:131-137), which is
 * GCounter::merge (src/gcounter.rs:58-62) and, on P and on N, PNCounter::merge
 * (src/pncounter.rs:90-95), in rank order, the fixed-order convention of
 * crdt_orswot_fold, crdt_lwwreg_fold and crdt_mvreg_fold. One launch: every
 * replica entry is read once, the output is written once, no intermediate
 * batch exists and the host is not synchronised. h_rows / h_reps are HOST
 * arrays of n_reps device pointers / views.
 *
 * crdt_clock_dense_fold: d_out[i][a] = max over r of h_rows[r][i][a], over
 * rows of n_slots words (n_actors for VClock and GCounter, 2 * n_actors for
 * PNCounter's [P|N] rows, as in crdt_dense_merge_host). Flat over n_obj *
 * n_slots words: R + 1 words of traffic per slot. d_out may be any h_rows[r]
 * (a word is read from every replica before it is written). n_reps == 1
 * copies through; n_reps == 2 gives crdt_vclock_dense_merge's bytes.
 *
 * crdt_clock_csr_fold: out[i] = the sorted union of object i's R runs with
 * the largest counter per actor. out.off[i] := the sum over r of
 * reps[r].off[i], out.len[i] := the union's length: the offsets, lengths and
 * entries the chain of crdt_vclock_csr_merge ends with. out.n_entries >= the
 * sum of the replicas' n_entries suffices (CRDT_ECAPACITY otherwise) and the
 * output is itself a valid (gapped) input batch. Object i's region is
 * [out.off[i], out.off[i] + the sum over r of reps[r].len[i]); regions are
 * disjoint whenever every replica is placed correctly. The kernel may use a
 * region as scratch: cells of it past out.len[i] are unspecified (as the
 * merge's gaps are); nothing outside the regions, out.off and out.len is
 * written, and no caller scratch is needed. n_reps == 1 copies the runs
 * through, checked; n_reps == 2 equals crdt_vclock_csr_merge in off, len, used
 * entries and codes. PNCounter is two calls, P and N. Runs of any length.
 *
 * CRDT_EINVAL, before any device work: null ctx, h_rows, h_reps or out; n_reps
 * 0 or > CRDT_CLOCK_FOLD_MAX_REPS; replicas whose n_obj differ; n_slots 0; a
 * null array with n_obj > 0 (a null act / ctr with n_entries > 0); a CSR out
 * array equal to a replica's array. n_obj == 0 is CRDT_OK and launches nothing.
 * Latched per object (out.len[i] = 0, every other object folded): CRDT_EINVAL
 * for a run of any replica out of its arrays or overlapping its neighbour
 * (off[i] + len[i] > off[i+1]) and for a region that does not fit
 * out.n_entries; CRDT_ENONCANON for a run of any replica that is not canonical
 * (actors not strictly increasing, a zero counter). For R > 2 this is the one
 * difference from the chain: the chain restarts an object's union from empty
 * after a step that met a bad run and goes on with the later replicas; the
 * fold leaves the object empty.
 *
 * Tiers, per object on the device, by T = the sum of its R lengths:
 *   T <= 64: the union is built in registers (one lane per entry);
 *   T <= CRDT_CLOCK_FOLD_STAGE_ENTRIES: the runs are staged in LDS. A wave's
 *     LDS is 14 B per entry (actor, counter, a u16 index) + 96 B = 7,264 B at
 *     512 entries; a block of 4 waves 29,056 B; 5 blocks, 20 waves (5 per
 *     SIMD), fit a CU's 160 KB (the kernel's 110 registers make it 4 per
 *     SIMD). 512 covers 8 replicas of the ~48-entry clocks measured below;
 *   longer: binary searches in HBM, the object's own region as scratch.
 *
 * Fold or chain (measured, 1M objects). Dense rows of 16
 * slots: the fold at every R — one crdt_vclock_dense_merge's time at R = 2
 * (0.998x, inside the merge's spread), 0.56x the chain of R - 1 merges at
 * R = 4, 0.45x at R = 8. CSR clocks of ~48 entries: the fold from R = 3 on —
 * 0.62x the chain at R = 4, 0.49x at R = 8, and no intermediate batches — but
 * at R = 2 call crdt_vclock_csr_merge: two such runs sum past 64 entries, so
 * the fold takes its LDS tier and 2.64x the time of the merge, which joins
 * runs of up to 64 entries a side in registers.
 * ------------------------------------------------------------------------ */
#define CRDT_CLOCK_FOLD_MAX_REPS 32
#define CRDT_CLOCK_FOLD_STAGE_ENTRIES 512
int crdt_clock_dense_fold(crdt_ctx* ctx, const uint64_t* const* h_rows, uint32_t n_reps, uint64_t* d_out,
                          size_t n_obj, uint32_t n_slots, void* stream);
int crdt_clock_csr_fold(crdt_ctx* ctx, const crdt_clock_csr* h_reps, uint32_t n_reps,
                        const crdt_clock_csr_out* out, void* stream);

/* ------------------------------------------------------------------------ *
 * Batched op path of the clocks and counters (clock_ops.hip): CmRDT::apply,
 * Causal::truncate, the reads, and the two primitives the reference builds
 * the rest from (subtract, intersection), on dense rows and on CSR runs.
 *
 * A batch of dots (or, for the get calls, of queried actors) grouped per
 * object; within an object the order never matters (witness is a max).
 *
 * Every call: CRDT_EINVAL (before any device work) for a null ctx, a null
 * struct, a null array with n_obj > 0 (a null op array whose count says it is
 * non-empty), n_actors == 0 (dense calls), an output aliasing an input.
 * Otherwise n_obj == 0 is CRDT_OK. Per-object faults latch on the context
 * (crdt_ctx_status) and leave the other objects untouched; nothing outside
 * the described arrays is read or written.
 * ------------------------------------------------------------------------ */
typedef struct crdt_clock_ops {   /* all device arrays */
  const uint64_t* obj_end;  /* n_obj: object i's ops are [obj_end[i-1], obj_end[i]) */
  const uint32_t* actor;    /* n_ops */
  const uint64_t* counter;  /* n_ops (unused by the get calls) */
  const uint32_t* dir;      /* n_ops, PNCounter only: 0 = Dir::Pos, 1 = Dir::Neg; else may be null */
  size_t n_ops;
} crdt_clock_ops;

/* Dense rows (the layout of crdt_vclock_dense_merge), in place on d_self.
 *
 * crdt_vclock_dense_apply / crdt_gcounter_apply: VClock::apply == witness
 * (src/vclock.rs:126-128, 159-163), GCounter::apply (src/gcounter.rs:53-55):
 * row[i][actor] = max(row[i][actor], counter) for each of object i's dots. A
 * repeated actor keeps its largest counter; a dot with counter 0 is a no-op;
 * rows of objects without ops are neither read nor written.
 * crdt_pncounter_apply: PNCounter::apply (src/pncounter.rs:82-87) on [P|N]
 * rows: dir 0 -> slot actor, dir 1 -> slot n_actors + actor.
 * Latched CRDT_ENONCANON: an actor >= n_actors, a dir above 1 (the op is
 * skipped, the object's other ops still apply), an object whose range
 * [obj_end[i-1], obj_end[i]) decreases or runs past n_ops (the object is
 * skipped; the others apply their ranges).
 * CRDT_EINVAL also for a null counter array (a null dir array, PNCounter)
 * with n_ops > 0, and for d_self equal to an op array. */
int crdt_vclock_dense_apply(crdt_ctx* ctx, uint64_t* d_self, const crdt_clock_ops* ops, size_t n_obj,
                            uint32_t n_actors, void* stream);
int crdt_gcounter_apply(crdt_ctx* ctx, uint64_t* d_self, const crdt_clock_ops* ops, size_t n_obj,
                        uint32_t n_actors, void* stream);
int crdt_pncounter_apply(crdt_ctx* ctx, uint64_t* d_self, const crdt_clock_ops* ops, size_t n_obj,
                         uint32_t n_actors, void* stream);

/* crdt_vclock_dense_truncate: Causal::truncate (src/vclock.rs:103-120):
 *   self[k] = min(self[k], other[k]) (absent is 0: an actor missing on either
 *   side disappears).
 * crdt_vclock_dense_subtract: VClock::subtract (src/vclock.rs:236-242):
 *   self[k] = other[k] >= self[k] ? 0 : self[k].
 * crdt_vclock_dense_intersection: VClock::intersection (src/vclock.rs:219-228):
 *   self[k] = self[k] == other[k] ? self[k] : 0.
 * Flat over n_obj * n_actors words like the merge (24 B of traffic per slot).
 * CRDT_EINVAL also for d_self == d_other. */
int crdt_vclock_dense_truncate(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                               uint32_t n_actors, void* stream);
int crdt_vclock_dense_subtract(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                               uint32_t n_actors, void* stream);
int crdt_vclock_dense_intersection(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                                   uint32_t n_actors, void* stream);

/* crdt_gcounter_value: GCounter::value (src/gcounter.rs:76-78): d_out[i] =
 * the wrapping u64 sum of row i.
 * crdt_pncounter_value: PNCounter::value (src/pncounter.rs:117-119) of [P|N]
 * rows: d_out[i] = (int64_t)sumP - (int64_t)sumN, wrapping.
 * CRDT_EINVAL also for d_out == d_rows. */
int crdt_gcounter_value(crdt_ctx* ctx, const uint64_t* d_rows, uint64_t* d_out, size_t n_obj, uint32_t n_actors,
                        void* stream);
int crdt_pncounter_value(crdt_ctx* ctx, const uint64_t* d_rows, int64_t* d_out, size_t n_obj, uint32_t n_actors,
                         void* stream);

/* crdt_vclock_dense_get: VClock::get (src/vclock.rs:206-210): d_out[j] =
 * row[i][queries.actor[j]] for object i's queries j (d_out has
 * queries.n_ops words; counter and dir are not read). An actor >= n_actors
 * reads 0 without latching (an absent actor is 0). VClock::inc (:182-185) is
 * get + 1, left to the caller. A query outside every object's range (an
 * obj_end decreasing or past n_ops latches CRDT_ENONCANON) is not written.
 * CRDT_EINVAL also for d_out equal to d_rows or to a query array. */
int crdt_vclock_dense_get(crdt_ctx* ctx, const uint64_t* d_rows, const crdt_clock_ops* queries, uint64_t* d_out,
                          size_t n_obj, uint32_t n_actors, void* stream);

/* CSR clocks (crdt_clock_csr / crdt_clock_csr_out above), never in place.
 * Placement and canonical-form checks and their latched codes are those of
 * crdt_vclock_csr_merge: a misplaced run latches CRDT_EINVAL, a non-canonical
 * run CRDT_ENONCANON, and out.len[i] is 0 in both cases.
 *
 * crdt_vclock_csr_truncate / _subtract / _intersection: a filter of self's
 * run by other's —
 *   truncate (src/vclock.rs:103-120) keeps actors present on both sides, with
 *     the smaller counter;
 *   subtract (:236-242) drops actors where other's counter is >= self's;
 *   intersection (:219-228) keeps actors whose counter is equal on both sides.
 * out.off[i] := self.off[i], out.len[i] <= self.len[i]; out.n_entries >=
 * self.n_entries suffices (CRDT_ECAPACITY otherwise) and the output is a
 * valid (gapped) input batch. CRDT_EINVAL also for self.n_obj != other.n_obj
 * and for an out array equal to an array of self or other.
 *
 * crdt_vclock_csr_apply / crdt_gcounter_csr_apply: out[i] = self's run after
 * witnessing object i's dots (VClock::apply src/vclock.rs:126-128, GCounter::
 * apply src/gcounter.rs:53-55). The op list is unsorted and may repeat
 * actors; a counter-0 dot creates no entry. out.off[i] := self.off[i] +
 * obj_end[i-1], out.len[i] <= self.len[i] + (ops of i); out.n_entries >=
 * self.n_entries + ops.n_ops suffices (CRDT_ECAPACITY otherwise). An object
 * without ops is copied through. An obj_end that decreases or runs past
 * n_ops latches CRDT_ENONCANON (out.len 0). ops.dir is not read. */
int crdt_vclock_csr_truncate(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                             const crdt_clock_csr_out* out, void* stream);
int crdt_vclock_csr_subtract(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                             const crdt_clock_csr_out* out, void* stream);
int crdt_vclock_csr_intersection(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                                 const crdt_clock_csr_out* out, void* stream);
int crdt_vclock_csr_apply(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_ops* ops,
                          const crdt_clock_csr_out* out, void* stream);
int crdt_gcounter_csr_apply(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_ops* ops,
                            const crdt_clock_csr_out* out, void* stream);

/* crdt_gcounter_csr_value: GCounter::value (src/gcounter.rs:76-78): d_out[i]
 * = the wrapping u64 sum of run i (0 for a run out of [0, n_entries), which
 * latches CRDT_EINVAL). Canonical form is not checked: a sum needs none.
 * crdt_vclock_csr_get: VClock::get (src/vclock.rs:206-210): d_out[j] = the
 * counter of queries.actor[j] in object i's run, by binary search (the run is
 * taken as sorted); an absent actor reads 0. */
int crdt_gcounter_csr_value(crdt_ctx* ctx, const crdt_clock_csr* self, uint64_t* d_out, void* stream);
int crdt_vclock_csr_get(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_ops* queries, uint64_t* d_out,
                        void* stream);

/* ------------------------------------------------------------------------ *
 * Orswot canonical record (one object = one contiguous, self-describing
 * record; a batch = a byte buffer + a u64 byte offset per object).
 *
 * The reference state is (src/orswot.rs:26-30)
 *     clock:    VClock<A>
 *     entries:  HashMap<M, VClock<A>>
 *     deferred: HashMap<VClock<A>, HashSet<M>>
 * and equality is structural (`#[derive(PartialEq)]`, src/orswot.rs:25). The
 * record is the canonical form of that state: hash-map order is replaced by
 * sorted order, so two states are equal iff their records are byte-equal.
 *
 * Record = header (32 B) followed by a MEMBER block and a DEFERRED block.
 * Every section is densely packed; the member block is zero-padded to a
 * multiple of 8 bytes and the record to a multiple of 16 bytes:
 *   u64 clk_ctr [n_clk]      top clock, DENSE: n_clk == n_actors, 0 = absent
 *   -- member block (entries: HashMap<M, VClock<A>>) --
 *   u64 mem_key [n_mem]      member keys, strictly increasing
 *   u64 dot_ctr [n_dot]      member clocks' counters, member-major
 *   u32 dot_act [n_dot]      member clocks' actors, strictly increasing per member
 *   u32 mem_dend[n_mem]      cumulative end of member m's dots (member m owns
 *                            dots [mem_dend[m-1], mem_dend[m]), mem_dend[-1]=0)
 *   (pad to 8)
 *   -- deferred block (deferred: HashMap<VClock<A>, HashSet<M>>) --
 *   u64 def_ctr [n_def_dot]  deferred clocks' counters, clock-major
 *   u64 def_key [n_def_mem]  deferred member sets, clock-major, each strictly increasing
 *   u32 def_act [n_def_dot]  deferred clocks' actors, strictly increasing per clock
 *   u32 def_dend[n_def]      cumulative end of deferred clock d's dots
 *   u32 def_mend[n_def]      cumulative end of deferred clock d's member keys
 *   (pad to 16)
 * SPARSE (CSR) top clock — header flags bit 0 (CRDT_ORSWOT_SPARSE_CLOCK), for
 * large actor universes (BASELINE.json configs[4]): the
 * top-clock section is instead
 *   u64 clk_ctr [n_clk]      counters of the clock's n_clk = nnz actors
 *   u32 clk_act [n_clk]      their actor ids, strictly increasing, < n_actors
 *   (pad to 8)
 * and everything after it is unchanged. A batch is either all dense (flags 0,
 * n_clk == n_actors) or all sparse (flags 1, counters > 0).
 * Canonical: every counter stored in a run is > 0, every member clock, every
 * deferred clock and every deferred member set is non-empty, and deferred
 * clocks are strictly increasing in CLOCK ORDER = lexicographic order of their
 * (actor, counter) sequences, a proper prefix ordering first.
 * ------------------------------------------------------------------------ */
typedef struct crdt_orswot_hdr {
  uint32_t size;      /* record bytes (header included), multiple of 16 */
  uint32_t n_clk;     /* dense top clock slots (== batch n_actors)      */
  uint32_t n_mem;
  uint32_t n_dot;
  uint32_t n_def;
  uint32_t n_def_dot;
  uint32_t n_def_mem;
  uint32_t flags;     /* 0 (dense top clock) or CRDT_ORSWOT_SPARSE_CLOCK  */
} crdt_orswot_hdr;

#define CRDT_ORSWOT_SPARSE_CLOCK 1u
/* Header flags bit 1: the record holds a member whose clock is EMPTY (an
 * empty run). Only Causal::truncate produces one (crdt_orswot_truncate: the
 * reference keeps such a member, src/orswot.rs:167-169); it is not a
 * canonical input of the merge, apply and codec entry points, which reject
 * it (CRDT_ENONCANON). */
#define CRDT_ORSWOT_EMPTY_MEMBER_CLOCK 2u

#define CRDT_ORSWOT_HDR_BYTES 32u
#define CRDT_RECORD_ALIGN 16u

/* Bytes of a record with these counts (header and padding included). */
size_t crdt_orswot_record_bytes(uint32_t n_clk, uint32_t n_mem, uint32_t n_dot,
                                uint32_t n_def, uint32_t n_def_dot, uint32_t n_def_mem);
/* Same for either clock form (flags: 0 or CRDT_ORSWOT_SPARSE_CLOCK). */
size_t crdt_orswot_record_bytes_ex(uint32_t n_clk, uint32_t n_mem, uint32_t n_dot,
                                   uint32_t n_def, uint32_t n_def_dot, uint32_t n_def_mem,
                                   uint32_t flags);

/* A batch of records: record i starts at d_base + d_off[i] (16-B aligned). */
typedef struct crdt_orswot_batch {
  const uint8_t* base;   /* device */
  const uint64_t* off;   /* device, n_obj entries */
  size_t n_obj;
  size_t bytes;          /* extent of base, for bounds checks */
} crdt_orswot_batch;

/*
 * out[i] := self[i].merge(&other[i])   — src/orswot.rs:87-157 incl.
 * apply_deferred (:235-243) / apply_remove (:195-211).
 *
 * The output record i is written at d_out_base + d_out_off[i] where
 * d_out_off[i] := self.off[i] + other.off[i] (written by the kernel). Because a
 * merged record is never larger than the two inputs together, the output
 * needs at most self.bytes + other.bytes bytes and no prefix scan: the output
 * batch (d_out_base, d_out_off) is itself a valid input batch (it may have
 * gaps between records; crdt_orswot_compact removes them).
 * PRECONDITION (checked on the device; a violation latches CRDT_EINVAL and
 * the offending objects are not written): on each side the records are in
 * increasing offset order and do not overlap, off[i] + size[i] <= off[i+1],
 * so that the output records cannot overlap either. Packed batches, merge
 * outputs (with gaps) and compacted batches all satisfy it.
 * `n_actors` is the dense top-clock width shared by every record.
 */
int crdt_orswot_merge(crdt_ctx* ctx, const crdt_orswot_batch* self,
                      const crdt_orswot_batch* other, uint8_t* d_out_base,
                      uint64_t* d_out_off, size_t out_bytes, uint32_t n_actors,
                      void* stream);

/* crdt_orswot_merge for either clock form: flags = 0 (dense top clocks,
 * n_actors slots) or CRDT_ORSWOT_SPARSE_CLOCK (CSR top clocks over an actor
 * universe of n_actors ids; the output records are sparse too). Same output
 * placement and bounds. */
int crdt_orswot_merge_ex(crdt_ctx* ctx, const crdt_orswot_batch* self,
                         const crdt_orswot_batch* other, uint8_t* d_out_base,
                         uint64_t* d_out_off, size_t out_bytes, uint32_t n_actors,
                         uint32_t flags, void* stream);

/* Same with host buffers: H2D, merge, D2H, synchronous (PCIe-inclusive path
 * used by a host `merge_batch(&mut [T], &[T])`). h_out_off receives offsets
 * into h_out_base (compacted, so h_out_bytes >= sum of merged record sizes
 * suffices; worst case h_self_bytes + h_other_bytes). */
int crdt_orswot_merge_host(crdt_ctx* ctx, const uint8_t* h_self_base,
                           const uint64_t* h_self_off, size_t self_bytes,
                           const uint8_t* h_other_base, const uint64_t* h_other_off,
                           size_t other_bytes, size_t n_obj, uint32_t n_actors,
                           uint8_t* h_out_base, uint64_t* h_out_off, size_t h_out_bytes,
                           size_t* h_out_used);

/* The replica fold, batched: out[i] := ((reps[0][i] ⊔ reps[1][i]) ⊔ reps[2][i])
 * ⊔ ... ⊔ reps[n_reps-1][i] — Orswot::merge (src/orswot.rs:87-157) in rank
 * order, the fold of replica anti-entropy (BASELINE.json configs[4]) — over
 * n_reps batches of the same n_obj objects: n_reps - 1 batched merges
 * (crdt_orswot_merge_ex) with the intermediate batches in a context-owned
 * buffer. flags: 0 (dense top clocks) or CRDT_ORSWOT_SPARSE_CLOCK. Output
 * record i at d_out_off[i] := sum_r reps[r].off[i] (written by the call);
 * out_bytes >= sum_r reps[r].bytes. Each batch: records in increasing offset
 * order, not overlapping (as crdt_orswot_merge). (A fused form — one wave
 * folding an object's records with the accumulator in LDS, no intermediate
 * batch in HBM — measured slower on config 5: the fold is bound by the joins,
 * not by the intermediate bytes; DESIGN.md.) */
int crdt_orswot_fold(crdt_ctx* ctx, const crdt_orswot_batch* reps, uint32_t n_reps, uint32_t n_actors,
                     uint32_t flags, uint8_t* d_out, uint64_t* d_out_off, size_t out_bytes, void* stream);

/* Deep canonical-form check of a batch on the device (sortedness, non-zero
 * counters, non-empty runs, section sizes). Result via crdt_ctx_status. */
int crdt_orswot_validate(crdt_ctx* ctx, const crdt_orswot_batch* batch,
                         uint32_t n_actors, void* stream);
int crdt_orswot_validate_ex(crdt_ctx* ctx, const crdt_orswot_batch* batch,
                            uint32_t n_actors, uint32_t flags, void* stream);

/* Remove gaps: copies records into d_dst contiguously; d_dst_off receives the
 * new offsets. d_scratch needs crdt_orswot_compact_scratch_bytes(n_obj). */
size_t crdt_orswot_compact_scratch_bytes(size_t n_obj);
int crdt_orswot_compact(crdt_ctx* ctx, const crdt_orswot_batch* src, uint8_t* d_dst,
                        uint64_t* d_dst_off, size_t dst_bytes, void* d_scratch,
                        void* stream);

/* ------------------------------------------------------------------------ *
 * Replica anti-entropy across GPUs over RCCL (xGMI) — SURVEY.md §8(b),(e);
 * BASELINE.json configs[3] (dense) and configs[4] (Orswot). One process (or
 * thread) per GPU, each holding a full replica of the same n objects. The
 * context owns one RCCL communicator:
 *   rank 0:     crdt_comm_unique_id(id), then the caller distributes the
 *               CRDT_COMM_ID_BYTES bytes to every rank (its own channel);
 *   every rank: crdt_comm_init(ctx, id, n_ranks, rank)     (collective).
 * Every collective entry point below must be called by every rank, in the
 * same order, on the stream each rank passes. A failure found on one rank
 * (bad batch, capacity, a non-canonical record) is returned by all ranks.
 * ------------------------------------------------------------------------ */
#define CRDT_COMM_ID_BYTES 128
int crdt_comm_unique_id(uint8_t* h_id);
int crdt_comm_init(crdt_ctx* ctx, const uint8_t* h_id, int n_ranks, int rank);
/* Also done by crdt_ctx_destroy. */
int crdt_comm_destroy(crdt_ctx* ctx);

/* *h_count := the number of ranks of the context's communicator (ncclCommCount). */
int crdt_comm_count(crdt_ctx* ctx, int* h_count);

/* Dense rows (VClock / GCounter / PNCounter rows, any width): d_rows[k] :=
 * max over ranks of d_rows[k], k < n_words, in place and in u64 order
 * (ncclAllReduce, ncclUint64, ncclMax; chunks of <= 1 GiB). It is
 * VClock::merge (src/vclock.rs:131-137) across replicas: a pointwise max,
 * commutative and associative, so the reduction order cannot change a bit. */
int crdt_replica_allreduce_max(crdt_ctx* ctx, uint64_t* d_rows, size_t n_words, void* stream);
/* The owner-shard variant: rank r receives in
 * d_shard the max over ranks of words [r n/N, (r+1) n/N) of d_rows (one
 * ncclReduceScatter, ncclUint64 + ncclMax); n_words must be a multiple of
 * the rank count. */
int crdt_replica_reduce_scatter_max(crdt_ctx* ctx, const uint64_t* d_rows, size_t n_words, uint64_t* d_shard,
                                    void* stream);

/* Orswot replicas: out[i] = ((r0[i] ⊔ r1[i]) ⊔ r2[i]) ⊔ ... ⊔ r_{N-1}[i], the
 * same bytes on every rank (the join is structurally non-commutative,
 * src/orswot.rs:98-103 vs :132-138, so the fold order is fixed: rank order).
 * Owner-sharded: the objects are split into N contiguous ranges; rank j
 * receives every replica's slice of range j point-to-point, folds it in rank
 * order with the batched merge kernel (crdt_orswot_merge_ex), compacts it,
 * and the folded ranges are exchanged back. Per rank: 1/N of the fold work
 * and about 2(N-1)/N of one replica's bytes sent and received.
 * `mine`: this rank's replica (the same n_obj on every rank; records in
 * increasing, non-overlapping offset order). The output is a packed batch,
 * record i at d_out + d_out_off[i], *h_out_used = its extent in bytes;
 * out_bytes >= crdt_orswot_replica_join_bound() suffices (the sum of every
 * rank's replica bytes, a collective). Synchronous: returns when the output
 * is complete on `stream`. A status an earlier launch on a rank's context
 * latched and the caller has not read (crdt_ctx_status) is that rank's error
 * in the join: every rank returns it, and the status is cleared. */
int crdt_orswot_replica_join_bound(crdt_ctx* ctx, const crdt_orswot_batch* mine, size_t* h_bound, void* stream);
int crdt_orswot_replica_join(crdt_ctx* ctx, const crdt_orswot_batch* mine, uint32_t n_actors, uint32_t flags,
                             uint8_t* d_out, uint64_t* d_out_off, size_t out_bytes, size_t* h_out_used,
                             void* stream);
/* The same owner-sharded join over a transport of the caller's (one process
 * per rank; e.g. gloo, MPI or a host network instead of RCCL) — no
 * communicator needed on ctx. The code above the transport is
 * crdt_orswot_replica_join's.
 *   allgather: blocking; every rank contributes n u64 (h_in), h_out receives
 *     n_ranks * n of them in rank order. Returns 0 or non-zero on failure.
 *   exchange: device transfers; every send {peer, src, bytes} is matched, in
 *     list order per peer, by that peer's recv {me, dst, bytes} of the same
 *     size (sends and recvs with peer == rank are local copies, k-th to
 *     k-th). src data is produced on `stream`; the transfers must be
 *     complete, or ordered before later work on `stream`, when it returns.
 *     Zero-byte entries move nothing. Returns 0 or non-zero on failure.
 * A transport failure returns CRDT_ECOMM. */
typedef struct crdt_xfer {
  int peer;
  const void* src;  /* device, sends */
  void* dst;        /* device, recvs */
  size_t bytes;
} crdt_xfer;
typedef struct crdt_transport {
  int n_ranks, rank;
  void* user;
  int (*allgather)(void* user, const uint64_t* h_in, size_t n, uint64_t* h_out);
  int (*exchange)(void* user, const crdt_xfer* sends, size_t n_sends, const crdt_xfer* recvs, size_t n_recvs,
                  void* stream);
} crdt_transport;
int crdt_orswot_replica_join_transport(crdt_ctx* ctx, const crdt_transport* transport,
                                       const crdt_orswot_batch* mine, uint32_t n_actors, uint32_t flags,
                                       uint8_t* d_out, uint64_t* d_out_off, size_t out_bytes, size_t* h_out_used,
                                       void* stream);
/* crdt_replica_allreduce_max over a transport of the caller's (above; no
 * communicator needed): rank j owns words [j n/N, (j+1) n/N) (the remainder
 * spread over the first ranks); each rank sends every peer its range, folds
 * the received copies of its own range with the dense max kernel, and sends
 * the result to every peer — the same bits as the RCCL all-reduce on every
 * rank (a pointwise max, src/vclock.rs:131-137). Uses the context's arena
 * for (N - 1) / N of the rows; synchronous: returns when d_rows is complete. */
int crdt_replica_allreduce_max_transport(crdt_ctx* ctx, const crdt_transport* transport, uint64_t* d_rows,
                                         size_t n_words, void* stream);
/* crdt_replica_reduce_scatter_max over a caller transport: rank r receives in
 * d_shard the max over ranks of words [r n/N, (r+1) n/N) of d_rows (n_words a
 * multiple of N) — its own copy of the range maxed with the N - 1 copies its
 * peers send it (the dense max kernel). Synchronous. */
int crdt_replica_reduce_scatter_max_transport(crdt_ctx* ctx, const crdt_transport* transport,
                                              const uint64_t* d_rows, size_t n_words, uint64_t* d_shard,
                                              void* stream);
/* The same owner-sharded join over n_replicas (<= 64) replicas resident on
 * this context's device: each replica is a virtual rank (a host thread with
 * its own context and stream) and device copies are the transport; the code
 * below the transport is crdt_orswot_replica_join's. For single-GPU
 * rehearsal and tests of the exchange. out_bytes >= the sum of the replicas'
 * (16-B aligned) bytes suffices. No communicator needed. */
int crdt_orswot_replica_join_local(crdt_ctx* ctx, const crdt_orswot_batch* replicas, uint32_t n_replicas,
                                   uint32_t n_actors, uint32_t flags, uint8_t* d_out, uint64_t* d_out_off,
                                   size_t out_bytes, size_t* h_out_used, void* stream);

/* ------------------------------------------------------------------------ *
 * Host-side helpers (no device work).
 * ------------------------------------------------------------------------ */

/* Synthetic Orswot pair batches by op simulation (Orswot::apply,
 * src/orswot.rs:61-85), identical for any sharding: object i draws from the
 * SplitMix64 stream seeded with (seed ^ i). Both sides share an ancestor
 * built from `ancestor_adds` adds of distinct members over all actors (each actor starting from a
 * random 40-bit counter base, as after a long history); side L then adds
 * with actors [0, n_actors/2), side R with [n_actors/2, n_actors).
 * Divergent ops per side: pct_add % adds, the rest removes with a read
 * context (Orswot::contains(m).rm_clock); in `pct_deferred_obj` % of objects,
 * `pct_future_rm` % of ops are removes with a FUTURE context (the side's clock
 * advanced on a remote actor), which defer (src/orswot.rs:197-203). In
 * `pct_shared_actor` % of objects side R also adds with actor 0 (the
 * weird_highlight_1 path, test/orswot.rs:84-92). */
typedef struct crdt_orswot_gen_params {
  uint32_t n_actors;         /* dense top-clock width (config 3: 16)            */
  uint32_t member_universe;  /* distinct member keys per object (config 3: 64)  */
  uint32_t ancestor_adds;    /* shared-history adds (config 3: 32)              */
  uint32_t min_div_ops;      /* divergent ops per side, uniform in [min, max]   */
  uint32_t max_div_ops;      /* (config 3: 4..16)                               */
  uint32_t pct_add;          /* (60)                                            */
  uint32_t pct_future_rm;    /* (10)                                            */
  uint32_t pct_deferred_obj; /* (8)                                             */
  uint32_t pct_shared_actor; /* (5)                                             */
} crdt_orswot_gen_params;

typedef struct crdt_orswot_gen crdt_orswot_gen;
/* Generates objects [first_obj, first_obj + n_obj) on n_threads host threads. */
int crdt_orswot_generate(uint64_t seed, size_t first_obj, size_t n_obj,
                         const crdt_orswot_gen_params* params, int n_threads,
                         crdt_orswot_gen** out);
/* side 0 = self (L), 1 = other (R) (or replica r): host base, u64 offsets (n_obj), bytes. */
int crdt_orswot_gen_side(const crdt_orswot_gen* g, int side, const uint8_t** h_base,
                         const uint64_t** h_off, size_t* bytes);
void crdt_orswot_gen_free(crdt_orswot_gen* g);

/* Replica sets for anti-entropy (config 5): per object, a shared ancestor of
 * `ancestor_adds` adds by actors of a per-object pool of `pool_actors` ids
 * drawn from [0, universe); each of the n_replicas replicas then applies
 * min..max divergent ops with its own `own_actors` ids (adds pct_add %,
 * read-context removes, and in pct_deferred_obj % of objects pct_future_rm %
 * removes whose context is advanced on another replica's actor, which
 * defer). Side r of the result (crdt_orswot_gen_side) is replica r. flags:
 * CRDT_ORSWOT_SPARSE_CLOCK encodes CSR top clocks (else dense, universe wide). */
typedef struct crdt_orswot_rep_params {
  uint32_t universe;         /* actor id universe (config 5: 1024)            */
  uint32_t pool_actors;      /* ancestor actors per object (48)               */
  uint32_t own_actors;       /* actors per replica per object (2)             */
  uint32_t member_universe;  /* (64)                                          */
  uint32_t ancestor_adds;    /* (48)                                          */
  uint32_t min_div_ops;      /* (4)                                           */
  uint32_t max_div_ops;      /* (16)                                          */
  uint32_t pct_add;          /* (60)                                          */
  uint32_t pct_future_rm;    /* (10)                                          */
  uint32_t pct_deferred_obj; /* (8)                                           */
} crdt_orswot_rep_params;
int crdt_orswot_generate_replicas(uint64_t seed, size_t first_obj, size_t n_obj,
                                  const crdt_orswot_rep_params* params, uint32_t n_replicas,
                                  uint32_t flags, int n_threads, crdt_orswot_gen** out);
/* The same replica sets, keeping only replicas [keep_first, keep_first +
 * keep_count) (side s of the result = replica keep_first + s): a rank
 * generates the replica it holds without encoding the others. */
int crdt_orswot_generate_replicas_subset(uint64_t seed, size_t first_obj, size_t n_obj,
                                         const crdt_orswot_rep_params* params, uint32_t n_replicas,
                                         uint32_t keep_first, uint32_t keep_count, uint32_t flags, int n_threads,
                                         crdt_orswot_gen** out);

/* ------------------------------------------------------------------------ *
 * Map<K, MVReg<u64, A>, A>::merge, batched (Map
 * src/map.rs:82-98, merge :191-268, apply_rm :336-349, apply_deferred
 * :323-333; MVReg truncate src/mvreg.rs:71-83 as the nested Causal value).
 * Keys are u64. Dense, fixed-capacity slabs, object i owning:
 *   clock[A]                            the map clock (0 = absent)
 *   n_keys, keys[kcap] ascending         entries (BTreeMap order)
 *   eclock[kcap][A]                      entry clocks
 *   mv_n[kcap], mv_clock[kcap][mcap][A], mv_val[kcap][mcap]   nested MVRegs (Vec order)
 *   n_def, dclock[dcap][A]               deferred removes in CLOCK ORDER
 *   dset_n[dcap], dset[dcap][scap]       their key sets, ascending
 * Only the used slots of the output are written (slots past a count keep
 * what the buffer held). Output capacities must be >= the sum of
 * both inputs' (kcap, mcap, dcap, scap); per side kcap <= 4096, mcap <= 128,
 * dcap <= 64, scap <= 4096, n_actors <= 128 (else CRDT_EINVAL); a merged map
 * past the output's capacities latches CRDT_ECAPACITY for that object.       */
typedef struct crdt_map_mvreg_slab {
  uint64_t* clock;
  uint32_t* n_keys;
  uint64_t* keys;
  uint64_t* eclock;
  uint32_t* mv_n;
  uint64_t* mv_clock;
  uint64_t* mv_val;
  uint32_t* n_def;
  uint64_t* dclock;
  uint32_t* dset_n;
  uint64_t* dset;
  uint32_t kcap, mcap, dcap, scap;
} crdt_map_mvreg_slab;
int crdt_map_mvreg_merge(crdt_ctx* ctx, const crdt_map_mvreg_slab* self, const crdt_map_mvreg_slab* other,
                         const crdt_map_mvreg_slab* out, size_t n_obj, uint32_t n_actors, void* stream);

/* ------------------------------------------------------------------------ *
 * Map<K, MVReg<u64, A>, A>::apply (CmRDT), batched: out[i] := self[i] after
 * Map::apply (src/map.rs:160-190) of each of object i's ops, in order, in the
 * slab's canonical form (keys ascending, MVReg values in Vec order, deferred
 * clocks in CLOCK ORDER, deferred key sets ascending). Only the used slots of
 * out are written. Object i's ops are [obj_end[i-1], obj_end[i]) of the op
 * arrays (all device arrays); op j's clock — an Rm's clock, an Up's Put
 * clock — is the (actor, counter) pairs [clk_end[j-1], clk_end[j]) of clk_act
 * / clk_ctr, actors strictly increasing, counters non-zero.
 *
 * The reference's rules, as applied:
 *  - Op::Nop (:165): nothing.
 *  - Op::Up, duplicate dot (:170-173): if map.clock.get(actor) >= counter the
 *    WHOLE op is skipped — no Put, no apply_deferred. A dot with counter 0 is
 *    therefore a no-op.
 *  - Op::Up otherwise (:175-187): the entry is taken out, or starts from an
 *    empty clock and an empty MVReg; entry.clock.witness(dot) (a max); the
 *    Put (MVReg::apply, src/mvreg.rs:158-186): an empty Put clock leaves the
 *    values untouched (:161-163) — the entry is still inserted, possibly with
 *    zero values; otherwise every value whose clock is <= the Put clock is
 *    dropped (:165), then (clock, val) is appended unless a remaining
 *    value's clock is strictly greater (:173-183); the entry is re-inserted;
 *    map.clock.witness(dot); apply_deferred.
 *  - Op::Rm -> apply_rm(key, clock) (:336-350): if !(clock <= map.clock) it
 *    is deferred — the key joins the set of an equal deferred clock, or a new
 *    deferred entry is inserted at its CLOCK ORDER position; then, if the
 *    entry exists, clock is subtracted from its clock and an emptied entry is
 *    removed, else MVReg::truncate(clock) (src/mvreg.rs:100-113), which may
 *    leave an entry with zero values. An empty Rm clock changes nothing.
 *  - apply_deferred (:325-333): all deferred entries are taken and cleared,
 *    and every (clock, key) goes through apply_rm again. With MVReg values
 *    each step is a subtract and subtracts commute: the result does not
 *    depend on the reference's HashMap order. The pass covers every deferred
 *    key, not only the updated one.
 *
 * CRDT_EINVAL (before any device work): a null ctx / self / ops / out;
 * n_actors == 0 or > 128; self capacities outside crdt_map_mvreg_merge's
 * per-side limits; an out capacity below self's or above kcap 8192, mcap 256,
 * dcap 128, scap 8192; a null slab array with n_obj > 0; a null op array its
 * count says is non-empty (obj_end: n_obj; kind .. clk_end: n_ops; clk_act,
 * clk_ctr: n_clk); out->clock == self->clock (the call is not in place, and
 * no out array may overlap a self array). n_obj == 0 is CRDT_OK; an object
 * without ops is copied through.
 * Latched per object (the other objects are unaffected, the object's output
 * row is unspecified): CRDT_ECAPACITY when at any step of its op list —
 * intermediate states count, as in crdt_orswot_apply — the state needs more
 * than out's kcap, mcap, dcap or scap; CRDT_ENONCANON for an input row the
 * merge rejects (a count above its capacity), obj_end / clk_end decreasing or
 * past n_ops / n_clk (nothing outside the op arrays is read), an unknown
 * kind, a dot actor >= n_actors, an op clock whose actors are not strictly
 * increasing or that holds a zero counter or an actor >= n_actors.          */
#define CRDT_MAP_OP_NOP 0u /* Op::Nop */
#define CRDT_MAP_OP_RM 1u  /* Op::Rm { clock, key } */
#define CRDT_MAP_OP_UP 2u  /* Op::Up { dot: (actor, counter), key, op: MVReg Op::Put { clock, val } } */
typedef struct crdt_map_mvreg_ops {
  const uint64_t* obj_end;   /* device, n_obj */
  const uint32_t* kind;      /* device, n_ops */
  const uint64_t* key;       /* device, n_ops (Rm, Up) */
  const uint32_t* actor;     /* device, n_ops (Up: the dot) */
  const uint64_t* counter;   /* device, n_ops (Up: the dot) */
  const uint64_t* val;       /* device, n_ops (Up: the Put's value) */
  const uint64_t* clk_end;   /* device, n_ops */
  const uint32_t* clk_act;   /* device, n_clk */
  const uint64_t* clk_ctr;   /* device, n_clk */
  size_t n_ops;
  size_t n_clk;
} crdt_map_mvreg_ops;
int crdt_map_mvreg_apply(crdt_ctx* ctx, const crdt_map_mvreg_slab* self, const crdt_map_mvreg_ops* ops,
                         const crdt_map_mvreg_slab* out, size_t n_obj, uint32_t n_actors, void* stream);

/* ------------------------------------------------------------------------ *
 * Map<K, Map<K, MVReg<u64, A>, A>, A>::merge, batched: the reference's own
 * Map test type (TestMap, test/map.rs:4-8; Map::merge src/map.rs:191-268 with
 * the inner map's merge and Causal::truncate :131-158 as the value's). Keys
 * are u64. Object i's outer map:
 *   clock[A], n_keys, keys[kcap] ascending, eclock[kcap][A]
 *   n_def, dclock[dcap][A] (CLOCK ORDER), dset_n[dcap], dset[dcap][scap]
 * and, for key slot k, its nested map as object i * kcap + k of `inner` (a
 * crdt_map_mvreg_slab of n_obj * kcap maps; its own limits as above).
 * Outer limits per side: kcap <= 4096, dcap <= 64, scap <= 4096; n_actors <=
 * 128; output capacities (outer and inner) >= the sums of the inputs' (else
 * CRDT_EINVAL); a result past them latches CRDT_ECAPACITY. d_scratch needs
 * crdt_map_map_merge_scratch_bytes(out, n_obj, n_actors) bytes (the per-slot
 * merge tasks and their truncating clocks). Only used slots
 * of the output are written. Where two deferred clocks of an inner map
 * become equal under truncation the later one's key set is kept (the
 * reference inserts into a HashMap there). */
typedef struct crdt_map_map_slab {
  uint64_t* clock;
  uint32_t* n_keys;
  uint64_t* keys;
  uint64_t* eclock;
  uint32_t* n_def;
  uint64_t* dclock;
  uint32_t* dset_n;
  uint64_t* dset;
  uint32_t kcap, dcap, scap;
  crdt_map_mvreg_slab inner;
} crdt_map_map_slab;
size_t crdt_map_map_merge_scratch_bytes(const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors);
int crdt_map_map_merge(crdt_ctx* ctx, const crdt_map_map_slab* self, const crdt_map_map_slab* other,
                       const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors, void* d_scratch,
                       size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Map<K, Map<K, MVReg<u64, A>, A>, A>::apply (CmRDT), batched — the op path
 * of TestMap: out[i] := self[i] after Map::apply (src/map.rs:160-190) of each
 * of object i's ops, in order, in the slab's canonical form (outer and inner:
 * keys ascending, MVReg values in Vec order, deferred clocks in CLOCK ORDER,
 * deferred key sets ascending). Only the used slots of out are written (the
 * inner rows of unused key slots not at all). Object i's ops are
 * [obj_end[i-1], obj_end[i]) of the op arrays (all device arrays); op j's
 * clock — an outer Rm's clock, an inner Rm's clock, an inner Up's Put clock —
 * is the pairs [clk_end[j-1], clk_end[j]) of clk_act / clk_ctr, actors
 * strictly increasing, counters non-zero. The inner Up's dot (actor2,
 * counter2) is a field of its own: Map::update makes it the outer dot, but
 * nothing in apply requires that.
 *
 * The reference's rules, as applied:
 *  - Op::Nop (:165): nothing.
 *  - Outer Op::Up, duplicate dot (:170-173): if map.clock.get(actor) >=
 *    counter the WHOLE op is skipped — no inner apply, no apply_deferred.
 *  - Outer Op::Up otherwise (:175-187): the entry is taken out, or starts from
 *    an empty clock and an empty inner map; entry.clock.witness(dot); the
 *    inner op runs on the inner map by the same Map::apply, against the inner
 *    map's own clock:
 *      inner Nop leaves it alone (a fresh key then holds an empty inner map,
 *        a legal state);
 *      inner Rm is the inner apply_rm (:336-350) with MVReg::truncate
 *        (src/mvreg.rs:100-113);
 *      inner Up is skipped when the inner clock has dot2 (:170-173; the outer
 *        op still counts), else the inner entry witnesses dot2 and takes the
 *        Put (src/mvreg.rs:158-186; an empty Put clock leaves the values
 *        untouched), the inner clock witnesses dot2 and the inner
 *        apply_deferred (:325-333) runs;
 *    the entry goes back in; map.clock.witness(dot); the outer apply_deferred.
 *  - Outer Op::Rm, and every step of the outer apply_deferred -> apply_rm
 *    (:336-350): if !(clock <= map.clock) it is deferred — the key joins an
 *    equal deferred clock's set, or a new entry is inserted at its CLOCK ORDER
 *    place; then, if the entry exists, clock is subtracted from its clock and
 *    an emptied entry is dropped, else the inner map takes
 *    Map::truncate(clock) (:131-158): each inner entry clock is subtracted, an
 *    emptied inner entry is dropped and any other takes MVReg::truncate; every
 *    inner deferred clock is subtracted and an emptied one is dropped; the
 *    inner clock is subtracted. An empty Rm clock changes nothing.
 *  - Inner deferred clocks under Map::truncate (:147-154): the subtract can
 *    reorder them and can make two equal; the result is put back in CLOCK
 *    ORDER, and where two become equal the key set of the later one (CLOCK
 *    ORDER before the subtract) is kept, as in crdt_map_map_merge (the
 *    reference inserts into a HashMap there).
 *  - The outer apply_deferred walks CLOCK ORDER, keys ascending. Apart from
 *    the collapse above the order is free: every step is a subtract.
 *
 * d_scratch: crdt_map_map_apply_scratch_bytes(out, n_obj, n_actors) bytes,
 * 16-byte aligned (an inner slab like out's, in which the edited inner maps
 * live until they are placed, and the per-key-slot placement tasks).
 *
 * CRDT_EINVAL (before any device work): a null ctx / self / ops / out;
 * n_actors == 0 or > 128; self capacities outside crdt_map_map_merge's
 * per-side limits (outer kcap 4096, dcap 64, scap 4096; inner kcap 4096, mcap
 * 128, dcap 64, scap 4096); an out capacity below self's or above twice that
 * limit, outer or inner; a null slab array or a null, misaligned or too small
 * scratch with n_obj > 0; a null op array its count says is non-empty
 * (obj_end: n_obj; kind .. clk_end: n_ops; clk_act, clk_ctr: n_clk);
 * out->clock == self->clock (the call is not in place, and no out array may
 * overlap a self array). n_obj == 0 is CRDT_OK; an object without ops is
 * copied through.
 * Latched per object (the other objects are unaffected, the object's output
 * row is unspecified): CRDT_ECAPACITY when at any step of its op list —
 * intermediate states count — the state needs more than one of out's seven
 * capacities; CRDT_ENONCANON for an input row the merge rejects (a count
 * above its capacity, outer or inner), obj_end / clk_end decreasing or past
 * n_ops / n_clk (nothing outside the op arrays is read), an unknown kind, an
 * actor >= n_actors in the dot, in an UP_UP's inner dot or in a clock, an op
 * clock whose actors are not strictly increasing or that holds a zero
 * counter.                                                                   */
#define CRDT_MAPMAP_OP_NOP 0u    /* Op::Nop */
#define CRDT_MAPMAP_OP_RM 1u     /* Op::Rm { clock, key } */
#define CRDT_MAPMAP_OP_UP_UP 2u  /* Op::Up { dot, key, op: Op::Up { dot2, key2, op: Put { clock, val } } } */
#define CRDT_MAPMAP_OP_UP_RM 3u  /* Op::Up { dot, key, op: Op::Rm { clock, key2 } } */
#define CRDT_MAPMAP_OP_UP_NOP 4u /* Op::Up { dot, key, op: Op::Nop } */
typedef struct crdt_map_map_ops {
  const uint64_t* obj_end;   /* device, n_obj */
  const uint32_t* kind;      /* device, n_ops */
  const uint64_t* key;       /* device, n_ops: the outer key (Rm, Up) */
  const uint32_t* actor;     /* device, n_ops: the outer dot (Up) */
  const uint64_t* counter;   /* device, n_ops */
  const uint64_t* key2;      /* device, n_ops: the inner key (UP_UP, UP_RM) */
  const uint32_t* actor2;    /* device, n_ops: the inner dot (UP_UP) */
  const uint64_t* counter2;  /* device, n_ops */
  const uint64_t* val;       /* device, n_ops: the Put's value (UP_UP) */
  const uint64_t* clk_end;   /* device, n_ops */
  const uint32_t* clk_act;   /* device, n_clk */
  const uint64_t* clk_ctr;   /* device, n_clk */
  size_t n_ops;
  size_t n_clk;
} crdt_map_map_ops;
size_t crdt_map_map_apply_scratch_bytes(const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors);
int crdt_map_map_apply(crdt_ctx* ctx, const crdt_map_map_slab* self, const crdt_map_map_ops* ops,
                       const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors, void* d_scratch,
                       size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Map<K, Orswot<u64, A>, A>::merge, batched (SURVEY.md §8(f) rank 3 as
 * written: src/map.rs:192-269 with the nested value's Causal::truncate,
 * src/orswot.rs:159-172, and Orswot::merge src/orswot.rs:87-157 for keys in
 * both maps). Keys and members are u64. Dense, fixed-capacity slabs, object
 * i owning:
 *   clock[A]                                   the map clock (0 = absent)
 *   n_keys, keys[kcap] ascending               entries (BTreeMap order)
 *   eclock[kcap][A]                            entry clocks
 *   nested Orswot per key:
 *     vclock[kcap][A]                          its top clock
 *     vn_mem[kcap], vmem[kcap][mcap]           members, ascending
 *     vmclock[kcap][mcap][A]                   member clocks (an all-zero row is
 *                                              an empty member clock, which
 *                                              truncate may leave in the
 *                                              reference; reachable states never
 *                                              hold one)
 *     vn_def[kcap], vdclock[kcap][vdcap][A]    deferred removes, CLOCK ORDER
 *     vdset_n[kcap][vdcap], vdset[kcap][vdcap][vscap]   their member sets, ascending
 *   n_def, dclock[dcap][A]                     the map's deferred removes, CLOCK ORDER
 *   dset_n[dcap], dset[dcap][scap]             their key sets, ascending
 * Only the used slots of the output are written: slots past a count keep
 * whatever the buffer held (a reader goes by the counts; zeroing them cost
 * ~10x the state's own bytes in writes). Per side kcap <= 4096, mcap <= 256,
 * vdcap, vscap, dcap <= 256, scap <= 4096, n_actors <= 128, and the
 * kernel's per-wave workspace — two nested sets of (mcap_s + mcap_o) member
 * rows and (vdcap_s + vdcap_o) deferred clocks of n_actors slots with their
 * member sets, plus 12 B per map deferred slot (dcap_s + dcap_o) — within
 * 64 KB
 * (else CRDT_EINVAL); output capacities must hold the result (else
 * CRDT_ECAPACITY is latched for that object). The map's deferred
 * removes are applied in CLOCK ORDER: the reference iterates a HashMap there
 * (src/map.rs:325-333) and, with Orswot values, two deferred clocks naming
 * the same key truncate its set in sequence, which can depend on that order
 * (DESIGN.md §5e); CLOCK ORDER is one of the reference's possible orders. */
typedef struct crdt_map_orswot_slab {
  uint64_t* clock;
  uint32_t* n_keys;
  uint64_t* keys;
  uint64_t* eclock;
  uint64_t* vclock;
  uint32_t* vn_mem;
  uint64_t* vmem;
  uint64_t* vmclock;
  uint32_t* vn_def;
  uint64_t* vdclock;
  uint32_t* vdset_n;
  uint64_t* vdset;
  uint32_t* n_def;
  uint64_t* dclock;
  uint32_t* dset_n;
  uint64_t* dset;
  uint32_t kcap, mcap, vdcap, vscap, dcap, scap;
} crdt_map_orswot_slab;
int crdt_map_orswot_merge(crdt_ctx* ctx, const crdt_map_orswot_slab* self, const crdt_map_orswot_slab* other,
                          const crdt_map_orswot_slab* out, size_t n_obj, uint32_t n_actors, void* stream);

/* ------------------------------------------------------------------------ *
 * Map<K, Orswot<u64, A>, A>::apply (CmRDT), batched: out[i] := self[i] after
 * Map::apply (src/map.rs:160-190) of each of object i's ops, in order, in the
 * slab's canonical form (keys ascending, members ascending, nested and map
 * deferred clocks in CLOCK ORDER, their sets ascending). Only the used slots
 * of out are written. The op batch is laid out as crdt_map_mvreg_ops: object
 * i's ops are [obj_end[i-1], obj_end[i]) of the op arrays (all device
 * arrays); op j's clock — a map Rm's clock, or the clock of an Up's nested
 * Orswot Rm — is the (actor, counter) pairs [clk_end[j-1], clk_end[j]) of
 * clk_act / clk_ctr, actors strictly increasing, counters non-zero (an
 * Up{Add}'s pairs are checked the same way and not used). The nested Add's
 * dot is the Up's dot, as Map::update builds it (src/map.rs:306-317 with
 * Orswot::add, src/orswot.rs:185-187): an Up whose nested Add carries another
 * dot cannot be expressed.
 *
 * The reference's rules, as applied:
 *  - Op::Nop (:165): nothing.
 *  - Op::Up, duplicate dot (:170-173): if map.clock.get(actor) >= counter the
 *    WHOLE op is skipped — no nested op, no apply_deferred.
 *  - Op::Up otherwise (:175-187): the entry is taken out, or starts from an
 *    empty clock and an empty Orswot; entry.clock.witness(dot); the nested op;
 *    the entry is re-inserted, even with an empty set; map.clock.witness(dot);
 *    apply_deferred.
 *  - nested Add (src/orswot.rs:66-79): skipped when the set's clock already
 *    has the dot (the entry clock and the map clock still witness it and the
 *    map's apply_deferred still runs); else the member's clock takes the dot
 *    (a max; an absent member is inserted in ascending position), the set's
 *    clock takes the dot, and the set's apply_deferred (:235-243) runs: every
 *    step of it is a subtract, so its order does not matter.
 *  - nested Rm -> apply_remove (src/orswot.rs:195-211): if !(clock <= the
 *    set's clock) it is deferred in the set — the member joins an equal
 *    deferred clock's set, or a new deferred entry is inserted at its CLOCK
 *    ORDER position; then clock is subtracted from the member's clock and an
 *    emptied member is dropped. An empty clock changes nothing, but the Up
 *    still happens.
 *  - Op::Rm -> apply_rm(key, clock) (src/map.rs:336-350): if !(clock <=
 *    map.clock) it is deferred in the map, as above with keys; then, if the
 *    entry exists, clock is subtracted from its clock and an emptied entry is
 *    removed, else Orswot::truncate(clock).
 *  - Orswot::truncate(clock) (src/orswot.rs:159-172), as in
 *    crdt_map_orswot_merge: members whose clock is <= clock are dropped; the
 *    set's clock is joined with clock; the set's apply_deferred runs under
 *    that clock, retiring the deferred clocks it now covers after removing
 *    their members; clock is subtracted from the set's clock and from every
 *    member clock.
 *  - apply_deferred (src/map.rs:325-333): all deferred entries are taken and
 *    cleared, and every (clock, key) goes through apply_rm again, in CLOCK
 *    ORDER and keys ascending — the order crdt_map_orswot_merge uses, and one
 *    of the orders the reference's HashMap can take. With Orswot values the
 *    order can change the result.
 *
 * CRDT_EINVAL (before any device work): a null ctx / self / ops / out;
 * n_actors == 0 or > 128; self capacities outside crdt_map_orswot_merge's
 * per-side limits; an out capacity below self's or above kcap 8192, mcap,
 * vdcap, vscap, dcap 512, scap 8192; the kernel's per-wave workspace — one
 * nested set of out's capacities: 8 * (mcap * (1 + n_actors) + vdcap *
 * (n_actors + vscap)) + 4 * (mcap + 2 * vdcap) bytes — above 60672 bytes
 * (64 KB less the kernel's op stage and key mirror); a null slab array with n_obj > 0; a null op
 * array its count says is non-empty (obj_end: n_obj; kind .. clk_end: n_ops;
 * clk_act, clk_ctr: n_clk); out->clock == self->clock (the call is not in
 * place, and no out array may overlap a self array). n_obj == 0 is CRDT_OK;
 * an object without ops is copied through.
 * Latched per object (the other objects are unaffected, the object's output
 * row is unspecified): CRDT_ECAPACITY when at any step of its op list —
 * intermediate states count: a fresh entry, member or deferred clock the
 * same op then removes still needs its slot — the state needs more than one
 * of out's six capacities; CRDT_ENONCANON for an input row the merge rejects
 * (a count above its capacity), obj_end / clk_end decreasing or past n_ops /
 * n_clk (nothing outside the op arrays is read), an unknown kind, a dot actor
 * >= n_actors, an op clock whose actors are not strictly increasing or that
 * holds a zero counter or an actor >= n_actors.                             */
#define CRDT_MAP_OP_UP_RM 3u /* Op::Up { dot, key, op: Orswot Op::Rm { clock, member } } */
/* for this call CRDT_MAP_OP_UP (2) is Op::Up { dot, key, op: Orswot Op::Add { dot, member } } */
typedef struct crdt_map_orswot_ops {
  const uint64_t* obj_end;   /* device, n_obj */
  const uint32_t* kind;      /* device, n_ops: NOP 0, RM 1, UP(Add) 2, UP_RM 3 */
  const uint64_t* key;       /* device, n_ops (Rm, Up) */
  const uint32_t* actor;     /* device, n_ops (Up: the dot) */
  const uint64_t* counter;   /* device, n_ops (Up: the dot) */
  const uint64_t* member;    /* device, n_ops (Up: the nested op's member) */
  const uint64_t* clk_end;   /* device, n_ops */
  const uint32_t* clk_act;   /* device, n_clk: a map Rm's clock, or an Up's nested Rm clock */
  const uint64_t* clk_ctr;   /* device, n_clk */
  size_t n_ops;
  size_t n_clk;
} crdt_map_orswot_ops;
int crdt_map_orswot_apply(crdt_ctx* ctx, const crdt_map_orswot_slab* self, const crdt_map_orswot_ops* ops,
                          const crdt_map_orswot_slab* out, size_t n_obj, uint32_t n_actors, void* stream);

/* ------------------------------------------------------------------------ *
 * Causal::truncate of the three Map types, batched (src/map.rs:131-158):
 * out[i] := self[i] after Map::truncate(d_clock[i]), d_clock dense
 * [n_obj][n_actors] with 0 = absent (as crdt_mvreg_truncate), in the slab's
 * canonical form (keys ascending, nested values in their own canonical form,
 * deferred clocks in CLOCK ORDER, sets ascending). Only the used slots of out
 * are written (the inner rows of unused key slots of a nested map not at
 * all). Not in place. With T = d_clock[i]:
 *  - Entry clocks (:134-141): every entry clock loses T — each actor whose
 *    counter is <= T's (VClock::subtract, src/vclock.rs:236-242). An entry
 *    whose clock becomes empty is dropped. Any other entry's value takes its
 *    own truncate(T):
 *      MVReg::truncate (src/mvreg.rs:100-113): every value clock loses T, an
 *        emptied value is dropped, order kept; an entry may be left with zero
 *        values.
 *      Orswot::truncate (src/orswot.rs:159-172), as in crdt_map_orswot_merge
 *        and crdt_map_orswot_apply: members whose clock is <= T are dropped;
 *        the set's clock is joined with T; the set's apply_deferred runs under
 *        that clock, retiring the deferred clocks it now covers after removing
 *        their members; T is subtracted from the set's clock and from every
 *        member clock — a member clock emptied by that last step stays, as an
 *        all-zero row. The set's deferred clocks are not subtracted.
 *      Map::truncate, these same rules, for the nested map.
 *  - Map deferred clocks (:147-154): every deferred clock loses T; an emptied
 *    one is dropped; the rest go back into CLOCK ORDER (the subtract can
 *    reorder them). Where two become equal the key set of the later one —
 *    CLOCK ORDER before the subtract — replaces the earlier one's, the rule of
 *    crdt_map_map_merge and crdt_map_map_apply (the reference inserts into a
 *    HashMap there).
 *  - Map clock (:156): the map clock loses T.
 *  - The reference runs no apply_deferred in truncate, and none runs here.
 *  - An all-zero T is the identity.
 *
 * crdt_map_map_truncate's d_scratch: crdt_map_map_truncate_scratch_bytes(out,
 * n_obj, n_actors) bytes, 16-byte aligned (per out key slot, the self inner
 * map it holds).
 *
 * CRDT_EINVAL (before any device work): a null ctx / self / out; a null
 * d_clock with n_obj > 0; n_actors == 0 or > 128; self capacities outside the
 * matching merge's per-side limits; an out capacity below self's or above the
 * matching apply's out limits; a null slab array with n_obj > 0; out->clock
 * == self->clock (no out array may overlap a self array); for the nested call
 * a null, misaligned or too small scratch with n_obj > 0; for Map<K, Orswot>
 * a per-wave workspace — one nested set of SELF's capacities, by
 * crdt_map_orswot_apply's formula: 8 * (mcap * (1 + n_actors) + vdcap *
 * (n_actors + vscap)) + 4 * (mcap + 2 * vdcap) bytes — above that call's
 * 60672 bytes. n_obj == 0 is CRDT_OK, null arrays included.
 * Latched per object (the other objects are unaffected, the object's output
 * row is unspecified): CRDT_ENONCANON for a count above its capacity, inner
 * maps included. Truncation never grows a count, so with out capacities >=
 * self's no object can latch CRDT_ECAPACITY.                                */
int crdt_map_mvreg_truncate(crdt_ctx* ctx, const crdt_map_mvreg_slab* self, const uint64_t* d_clock,
                            const crdt_map_mvreg_slab* out, size_t n_obj, uint32_t n_actors, void* stream);
int crdt_map_orswot_truncate(crdt_ctx* ctx, const crdt_map_orswot_slab* self, const uint64_t* d_clock,
                             const crdt_map_orswot_slab* out, size_t n_obj, uint32_t n_actors, void* stream);
size_t crdt_map_map_truncate_scratch_bytes(const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors);
int crdt_map_map_truncate(crdt_ctx* ctx, const crdt_map_map_slab* self, const uint64_t* d_clock,
                          const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors, void* d_scratch,
                          size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * VClock partial order and MVReg merge, batched.
 * crdt_vclock_partial_cmp: d_out[i] = partial_cmp(a[i], b[i])
 * (src/vclock.rs:59-71) over dense rows u64[n][n_actors], 0 = absent:
 * 0 Equal, 1 Greater (b <= a), -1 Less (a <= b), 2 None (concurrent).
 * crdt_mvreg_merge: MVReg<u64, A>::merge (src/mvreg.rs:121-153) over slabs
 * of `cap` (clock row, value) slots per object, d_*_n[i] slots in use; the
 * output keeps the reference's order (self's survivors, then other's) and
 * zero-fills unused slots. cap <= 1024 per side (registers of <= 64 slots
 * per side whose rows fit 60 KB of LDS per wave take the fast kernel, the
 * rest a one-wave-per-pair kernel reading the rows from HBM; a wave's LDS is
 * 8 (self_cap + other_cap) n_actors + self_cap other_cap + other_cap^2 +
 * out_cap bytes, rounded up to 16, and a block holds as many waves, 4 at the
 * most, as 60 KB allow); more survivors than out_cap latch CRDT_ECAPACITY, a
 * count above its side's capacity CRDT_ENONCANON. Both are latched per
 * object: that object's output is left unwritten and every other object is
 * merged as usual. n_obj == 0 is CRDT_OK and launches nothing, null arrays
 * included.                                                                 */
int crdt_vclock_partial_cmp(crdt_ctx* ctx, const uint64_t* d_a, const uint64_t* d_b, size_t n,
                            uint32_t n_actors, int8_t* d_out, void* stream);
int crdt_mvreg_merge(crdt_ctx* ctx, const uint32_t* d_self_n, const uint64_t* d_self_clk,
                     const uint64_t* d_self_val, uint32_t self_cap, const uint32_t* d_other_n,
                     const uint64_t* d_other_clk, const uint64_t* d_other_val, uint32_t other_cap,
                     uint32_t* d_out_n, uint64_t* d_out_clk, uint64_t* d_out_val, uint32_t out_cap,
                     size_t n_obj, uint32_t n_actors, void* stream);

/* ------------------------------------------------------------------------ *
 * crdt_mvreg_fold: out[i] = reps[0][i].merge(reps[1][i]).merge(reps[2][i])...
 * (src/mvreg.rs:121-153) in rank order, the fixed-order convention of
 * crdt_orswot_fold and crdt_lwwreg_fold, over crdt_mvreg_merge's slabs. One
 * launch: every replica's used slots are read once, the output is written
 * once, no intermediate register goes through HBM and the host is not
 * synchronised. h_reps is a HOST array of n_reps views. The output follows
 * the merge's convention (survivors in the reference's order, every unused
 * slot of d_out_clk / d_out_val zero-filled); n_reps == 1 copies replica 0
 * through, n_reps == 2 gives crdt_mvreg_merge's bytes. No slot past n[i] of
 * any replica takes part (the pipeline may load it, inside the slab, as the
 * merge's does).
 *
 * The rule, with (r, k) for used slot k of replica r and `>` for strictly
 * greater under VClock::partial_cmp: (r, k) is dropped when a used slot of
 * another replica is > it (a slot only its own replica dominates is kept, as
 * merge keeps it); otherwise it is kept when r == 0 (duplicates inside
 * replica 0 too); otherwise it is dropped when an equal clock sits at an
 * earlier slot of replica r, or in an earlier replica while no slot of
 * replica r is > this clock; survivors come out in (r, k) order.
 *
 * CRDT_EINVAL, before any device work: null ctx or h_reps; n_reps 0 or >
 * CRDT_MVREG_MAX_REPS; any cap 0 or > 1024; T = the caps' sum > 2048; out_cap
 * 0 or > 2048; n_actors 0; a null array with n_obj > 0; an output array equal
 * to a replica's array (not in place). n_obj == 0 is CRDT_OK, launches and
 * writes nothing, null arrays included (the capacities are still checked).
 * Latched per object as in the merge (its output left unwritten, every other
 * object folded): CRDT_ENONCANON for any n[r][i] > cap_r, CRDT_ECAPACITY for
 * more survivors than out_cap — the final count; the chain's intermediate
 * registers do not exist here.
 *
 * Tiers: T <= 64 and a wave's LDS of 8 T n_actors + 18 T bytes, rounded
 * up to 16, within 60 KB take the fast kernel (one wave per register, as
 * many waves per block, 4 at the most, as 60 KB allow); everything else a
 * one-wave-per-register kernel comparing the rows in HBM.
 *
 * Fold or chain (measured, 4M registers, 16 actors, 4 slots per replica,
 * DESIGN.md §5v): the fold is the faster at every R measured — 0.74x one
 * crdt_mvreg_merge at R = 2, 0.44x the chain of R - 1 merges at R = 4 and
 * 0.29x at R = 8 — and needs no intermediate slabs.
 * ------------------------------------------------------------------------ */
#define CRDT_MVREG_MAX_REPS 32
typedef struct crdt_mvreg_view {   /* one replica's registers, device arrays, crdt_mvreg_merge's slab */
  const uint32_t* n;    /* [n_obj] slots in use */
  const uint64_t* clk;  /* [n_obj][cap][n_actors], 0 = absent */
  const uint64_t* val;  /* [n_obj][cap] */
  uint32_t cap;
} crdt_mvreg_view;
int crdt_mvreg_fold(crdt_ctx* ctx, const crdt_mvreg_view* h_reps, uint32_t n_reps,
                    uint32_t* d_out_n, uint64_t* d_out_clk, uint64_t* d_out_val, uint32_t out_cap,
                    size_t n_obj, uint32_t n_actors, void* stream);

/* ------------------------------------------------------------------------ *
 * MVReg<u64, A> op path, batched, over crdt_mvreg_merge's slabs (n[i] slots
 * in use, clk[i][cap][n_actors] dense rows with 0 = absent, val[i][cap], Vec
 * order). Outputs follow the merge's convention: survivors in order, every
 * unused slot of d_out_clk / d_out_val zero-filled. Not in place.
 *
 * crdt_mvreg_apply: out[i] = self[i] after object i's Op::Put list in order
 * (CmRDT::apply, src/mvreg.rs:158-186). The op batch is crdt_map_mvreg_ops
 * without the map fields: object i owns ops [obj_end[i-1], obj_end[i]), op j
 * the clock pairs [clk_end[j-1], clk_end[j]) of clk_act / clk_ctr (actors
 * strictly increasing and < n_actors, counters > 0).
 *   - a Put with an empty clock (no pairs) leaves the register unchanged
 *     (:161-163);
 *   - any other Put first drops every value whose clock is <= the Put clock
 *     pointwise, equal clocks included (:165), order kept; then appends
 *     (clock, val) unless a remaining clock is strictly greater (:173-183).
 *     A Put may drop a value and still not be added.
 *   Input rows are taken as given: an all-zero stored row is <= every
 *   non-empty Put clock and is dropped by it.
 * crdt_mvreg_truncate: Causal::truncate (src/mvreg.rs:100-113) of register i
 * by d_clock[i] (dense [n_obj][n_actors], 0 = absent): every row loses each
 * actor whose counter is <= the truncating clock's (VClock::subtract,
 * src/vclock.rs:236-242); a slot whose row becomes all zero is dropped, order
 * kept. An all-zero truncating row is the identity.
 * crdt_mvreg_read_clock: d_out_clock[i] = read().add_clock (src/mvreg.rs:
 * 201-222), the pointwise max over the n[i] used rows (all zero for an empty
 * register); slots past n[i] are not read.
 *
 * CRDT_EINVAL (before any device work): a null ctx; a null ops struct
 * (crdt_mvreg_apply; also with n_obj == 0: the struct is always read); a
 * null array with n_obj > 0; n_actors == 0; self_cap == 0 or > 1024; out_cap
 * < self_cap or > 2048 (crdt_mvreg_read_clock: cap == 0 only, any cap above
 * is taken); a null op array whose count says it is non-empty; an output
 * pointer equal to its input pointer. Otherwise n_obj == 0 is CRDT_OK, null
 * arrays included. An object without ops is copied through, zero-filled to
 * out_cap.
 * Latched per object (crdt_ctx_status; the other objects are unaffected, the
 * object's output is unspecified): CRDT_ECAPACITY when any step of its op
 * list needs more than out_cap slots (intermediate states count; the drop of
 * a Put precedes its append); CRDT_ENONCANON for n[i] > cap, obj_end /
 * clk_end decreasing or past n_ops / n_clk (nothing outside the op arrays is
 * read), or an op clock with actors not strictly increasing, a zero counter
 * or an actor >= n_actors.
 * Registers of out_cap <= 64 slots whose [out_cap][n_actors] block fits 60 KB
 * of LDS per wave take the fast kernel; the rest a one-wave-per-register
 * kernel that edits the output block in HBM.                               */
typedef struct crdt_mvreg_ops {      /* all device arrays */
  const uint64_t* obj_end;  /* n_obj: object i's ops are [obj_end[i-1], obj_end[i]) */
  const uint64_t* val;      /* n_ops: the Put's value */
  const uint64_t* clk_end;  /* n_ops: op j's clock = pairs [clk_end[j-1], clk_end[j]) */
  const uint32_t* clk_act;  /* n_clk: actors strictly increasing within an op */
  const uint64_t* clk_ctr;  /* n_clk: non-zero */
  size_t n_ops, n_clk;
} crdt_mvreg_ops;
int crdt_mvreg_apply(crdt_ctx* ctx, const uint32_t* d_self_n, const uint64_t* d_self_clk,
                     const uint64_t* d_self_val, uint32_t self_cap, const crdt_mvreg_ops* ops,
                     uint32_t* d_out_n, uint64_t* d_out_clk, uint64_t* d_out_val, uint32_t out_cap,
                     size_t n_obj, uint32_t n_actors, void* stream);
int crdt_mvreg_truncate(crdt_ctx* ctx, const uint32_t* d_self_n, const uint64_t* d_self_clk,
                        const uint64_t* d_self_val, uint32_t self_cap, const uint64_t* d_clock,
                        uint32_t* d_out_n, uint64_t* d_out_clk, uint64_t* d_out_val, uint32_t out_cap,
                        size_t n_obj, uint32_t n_actors, void* stream);
int crdt_mvreg_read_clock(crdt_ctx* ctx, const uint32_t* d_n, const uint64_t* d_clk, uint32_t cap,
                          uint64_t* d_out_clock, size_t n_obj, uint32_t n_actors, void* stream);

/* ------------------------------------------------------------------------ *
 * Batched op path: CmRDT::apply for Orswot (src/orswot.rs:61-85; Op enum
 * :38-53): out[i] = self[i] after applying object i's ops in order.
 *   Op::Add { dot: (actor, counter), member }   kind CRDT_OP_ADD
 *   Op::Rm  { clock, member }                   kind CRDT_OP_RM; clock i is
 *     pairs [clk_end[i-1], clk_end[i]) of clk_act / clk_ctr (canonical:
 *     actors strictly increasing, counters > 0; Add ops own no pairs)
 * Object i's ops are [obj_end[i-1], obj_end[i]). Record i of the output is
 * written at d_out_off[i] = self.off[i] + P*(ops before i) + 16*(clock pairs
 * before i) + 32*i (set by the call), P = 32 for dense top clocks and 48 for
 * CSR ones (an Add may bring a new actor, member and dot: 36 B), so
 * out_bytes >= self.bytes + P*n_ops + 16*n_clk + 32*n_obj suffices.
 * PRECONDITION: self's records do not overlap and are in increasing offset
 * order (as any packed or merged batch); a record that would outgrow its own
 * span self.size + P*ops + 16*pairs + 32 latches CRDT_ECAPACITY and is not
 * written. Limits per object, at every step of its op list (past one:
 * CRDT_ECAPACITY, the object is not written): <= 2048 top-clock entries (dense:
 * n_actors <= 2048), <= 4096 members, <= 16384 dots, <= 2048 pairs in an Rm
 * clock, <= 256 deferred clocks with <= 4096 entries and <= 4096 members in
 * all. (Objects are joined in an 8 KB LDS workspace, those that outgrow it in
 * a 16 KB one, the rest in an HBM workspace: the limits are the last one's.) */
#define CRDT_OP_ADD 0u
#define CRDT_OP_RM 1u
typedef struct crdt_orswot_ops {
  const uint64_t* obj_end;   /* device, n_obj  */
  const uint32_t* kind;      /* device, n_ops  */
  const uint64_t* member;    /* device, n_ops  */
  const uint32_t* actor;     /* device, n_ops (Add) */
  const uint64_t* counter;   /* device, n_ops (Add) */
  const uint64_t* clk_end;   /* device, n_ops  */
  const uint32_t* clk_act;   /* device, n_clk  */
  const uint64_t* clk_ctr;   /* device, n_clk  */
  size_t n_ops;
  size_t n_clk;
} crdt_orswot_ops;
int crdt_orswot_apply(crdt_ctx* ctx, const crdt_orswot_batch* self, const crdt_orswot_ops* ops,
                      uint32_t n_actors, uint32_t flags, uint8_t* d_out, uint64_t* d_out_off,
                      size_t out_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Batched read path (read.hip): the reference's third verb, read -> ctx -> op.
 *   Orswot::contains (src/orswot.rs:214-224), Orswot::value (:227-233),
 *   Map::get (src/map.rs:291-302), Map::len (:282-288), and the contexts a
 *   ReadCtx derives (src/ctx.rs:45-60): derive_rm_ctx().clock = rm_clock,
 *   derive_add_ctx(actor) = { clock: add_clock with the dot witnessed, dot:
 *   (actor, add_clock.get(actor) + 1) }.
 * Queries are grouped per object like every op batch; a read changes nothing,
 * so every query of a batch sees the same object. Per query:
 *                 KEY (contains / get)             ALL (value / len)
 *   val           1 present, 0 absent              members / entries
 *   slot          the key's index, else NO_SLOT    NO_SLOT
 *   add_clock     the top / map clock              the top / map clock
 *   rm_clock      the member's / entry's clock     the top / map clock
 *                 (empty if absent)
 *   list          -                                the members / keys, ascending
 *                                                  (value() is a HashSet in the
 *                                                  reference; this is the
 *                                                  record's own order)
 * Two calls, like the egest codec: *_sizes writes the lengths (any array of
 * crdt_read_sizes may be null = not wanted, and what is not wanted is not
 * read: without add_len and dot_ctr the top clock is never touched; with an
 * actor and dot_ctr only, a dense clock costs that actor's word); the caller
 * takes the inclusive prefix sums of the lengths it wants; the write call puts
 * query j's pairs at [end[j-1], end[j]) of the group's arrays. A group whose
 * *_end is null is skipped. The pair arrays are in the op-clock form of
 * crdt_orswot_ops, crdt_mvreg_ops and crdt_map_*_ops (clk_end / clk_act /
 * clk_ctr: actors strictly increasing, counters > 0): rm_* of a batch of
 * contains queries are the clocks of the Op::Rm's of the same members in the
 * same order, add_* the Put clocks of Op::Up's, dot_ctr the dots' counters.
 *
 * crdt_orswot_read*: record batches with dense top clocks (flags 0) or
 * CRDT_ORSWOT_SPARSE_CLOCK ones; a batch with gaps is valid input, and so is
 * a record carrying CRDT_ORSWOT_EMPTY_MEMBER_CLOCK (contains of such a member:
 * val 1, an empty rm clock — entries.get returns Some(empty)). No per-object
 * limit beyond the record format's. add_len of a dense top clock is the count
 * of its non-zero slots, of a sparse one n_clk, plus one for a new actor.
 * crdt_map_read*: the four outer arrays the three Map slabs share (the view);
 * get: add_clock = the map clock, rm_clock = the entry clock; len: both are
 * the map clock. n_actors <= 128; kcap <= 8192, the largest slab an engine
 * call can produce. `slot` makes the nested read get(k1).val.get(k2) a second
 * call on `inner` with object i * kcap + slot.
 * crdt_map_mvreg_get: the val: Option<MVReg> of Map::get for Map<u64, MVReg>:
 * query j's register is copied into row j of a slab in crdt_mvreg_merge's
 * layout (d_out_n[n_q], d_out_clk[n_q][out_cap][n_actors], d_out_val[n_q]
 * [out_cap]; Vec order, unused slots zero-filled), ready for crdt_mvreg_merge,
 * crdt_mvreg_apply and crdt_mvreg_read_clock. An absent key and an ALL query
 * give n = 0. Only kind and key of the queries are read.
 * crdt_map_orswot_get*: the val of Map::get for Map<u64, Orswot> as a batch
 * of canonical records, two calls like the ingest codec. *_get_sizes writes
 * d_sizes[j], the bytes of query j's record (a multiple of 16), and, if
 * d_present is not null, 1 where the record is the key's value; the caller
 * places the records at 16-B aligned offsets (an exclusive scan of the sizes);
 * the write call puts record j at d_out + d_out_off[j]. (d_out, d_out_off, n_q,
 * out_bytes) is then a crdt_orswot_batch of n_q records with dense top clocks
 * (n_clk == n_actors, flags 0), valid input wherever a merge output is. The
 * record is the canonical form of the slab value: clk = the vclock row,
 * mem_key = vmem[0, vn_mem), member m's dots = the non-zero slots of vmclock[m]
 * (actors ascending), mem_dend their cumulative ends, the deferred clocks = the
 * non-zero slots of vdclock[d] in the slab's own CLOCK ORDER, their sets =
 * vdset[d][0, vdset_n[d]); padding bytes are zero. A member whose vmclock row
 * is all zero is kept as an empty run and the header gets
 * CRDT_ORSWOT_EMPTY_MEMBER_CLOCK. An absent key and an ALL query give present
 * 0 and the record of Orswot::default() (a header and a zero clock): what
 * Map::update hands its closure for a missing key; the batch stays dense in
 * n_q. The write call counts again: it never trusts the sizes call.
 * crdt_map_map_get: the val of get for the nested map: query j's inner map
 * (object i * kcap + slot of `inner`) is copied into row j of `out`, a
 * crdt_map_mvreg_slab of n_q rows that crdt_map_mvreg_merge / _apply /
 * _truncate / _to_bincode and crdt_map_read accept. The counts and the clock
 * row are always written, otherwise only the used slots (the Map slabs'
 * convention). An absent key and an ALL query give present 0, n_keys = n_def
 * = 0 and a zero clock: Map::default(). out's capacities may exceed inner's.
 * Both read only obj_end, kind and key of the queries, and a located value by
 * its used counts, never by its capacities.
 *
 * CRDT_EINVAL (before any device work): a null ctx or struct; with n_obj > 0 a
 * null batch / view array or obj_end; with n_q > 0 a null kind or key, (write
 * call) a wanted group's null array, (crdt_map_mvreg_get) a null output or
 * nested array; n_actors == 0 (maps: or > 128); kcap == 0 or > 8192; flags
 * other than 0 or CRDT_ORSWOT_SPARSE_CLOCK; an output array equal to an input
 * array; out_cap < slab.mcap; (crdt_map_orswot_get*, crdt_map_map_get) with
 * n_obj > 0 a null array of those the call reads, with n_q > 0 a null d_sizes,
 * d_out or array of `out`, a null d_out_off, an `out` capacity below inner's.
 * Otherwise n_obj == 0 is CRDT_OK.
 * Latched (crdt_ctx_status), the other queries and objects unaffected:
 *   CRDT_ENONCANON  an obj_end that decreases or runs past n_q (the object's
 *                   queries are not written, as in crdt_vclock_dense_get); a
 *                   record whose header counts do not fit its extent, whose
 *                   extent leaves [0, bytes) or whose clock form is not the
 *                   batch's, a map row with n_keys > kcap, an unknown kind
 *                   among the object's queries (every size of the object's
 *                   queries is 0, slot NO_SLOT); an actor >= n_actors other than
 *                   NO_ACTOR, and an actor whose counter is 2^64 - 1, where
 *                   the reference's inc overflows (src/vclock.rs:182-185):
 *                   dot_ctr 0, the query answered as without an actor;
 *                   crdt_map_mvreg_get: a register count above mcap (n = 0).
 *                   crdt_map_orswot_get*, crdt_map_map_get: a located value
 *                   whose counts exceed its capacities (vn_mem > mcap, vn_def
 *                   > vdcap, vdset_n > vscap; n_keys, mv_n, n_def or dset_n
 *                   above inner's) or that a record cannot hold (an all-zero
 *                   deferred clock row, an empty deferred set): the query gets
 *                   the default record or row and present 0, in both calls;
 *                   an unknown kind gives the object's queries the same.
 *   CRDT_ECAPACITY  (write call) a span end[j] - end[j-1] that is not the
 *                   query's length or leaves [0, n): the query's group is not
 *                   written; nothing outside the arrays is touched.
 *                   crdt_map_orswot_get: a d_out_off[j] that is not 16-B
 *                   aligned or whose record leaves [0, out_bytes): that record
 *                   is not written; nothing outside d_out is touched.
 * Sortedness is taken as given (as crdt_vclock_csr_get): no deep validation.
 * ------------------------------------------------------------------------ */
#define CRDT_READ_KEY 0u            /* Orswot::contains(member) / Map::get(key)            */
#define CRDT_READ_ALL 1u            /* Orswot::value()          / Map::len()               */
#define CRDT_READ_NO_ACTOR 0xFFFFFFFFu
#define CRDT_READ_NO_SLOT  0xFFFFFFFFu
typedef struct crdt_read_queries {  /* device arrays */
  const uint64_t* obj_end;  /* n_obj: object i's queries are [obj_end[i-1], obj_end[i]) */
  const uint32_t* kind;     /* n_q */
  const uint64_t* key;      /* n_q: member / map key (KEY queries)                      */
  const uint32_t* actor;    /* n_q, or null: the actor to derive an AddCtx for          */
  size_t n_q;
} crdt_read_queries;
typedef struct crdt_read_sizes {    /* device, n_q each, written by the *_sizes call; any may be null = not wanted */
  uint64_t* val;       /* KEY: 1 present / 0 absent.  ALL: number of members / entries  */
  uint32_t* slot;      /* KEY: index of the key among the object's members / entries, else NO_SLOT */
  uint64_t* dot_ctr;   /* derive_add_ctx(actor).dot.counter = add_clock.get(actor) + 1; 0 without an actor */
  uint32_t* add_len;   /* pairs of AddCtx.clock (add_clock with that dot witnessed); of add_clock itself without an actor */
  uint32_t* rm_len;    /* pairs of rm_clock: KEY: the member's / entry's clock (0 if absent); ALL: the top / map clock */
  uint32_t* list_len;  /* ALL: members / keys listed (= val); KEY: 0                    */
} crdt_read_sizes;
typedef struct crdt_read_out {      /* device; a group whose *_end is null is skipped */
  const uint64_t* add_end; uint32_t* add_act; uint64_t* add_ctr; size_t n_add;
  const uint64_t* rm_end;  uint32_t* rm_act;  uint64_t* rm_ctr;  size_t n_rm;
  const uint64_t* list_end; uint64_t* list_key; size_t n_list;   /* ascending */
} crdt_read_out;
typedef struct crdt_map_read_view {
  const uint64_t* clock; const uint32_t* n_keys; const uint64_t* keys; const uint64_t* eclock; uint32_t kcap;
} crdt_map_read_view;
int crdt_orswot_read_sizes(crdt_ctx* ctx, const crdt_orswot_batch* batch, const crdt_read_queries* queries,
                           uint32_t n_actors, uint32_t flags, const crdt_read_sizes* sizes, void* stream);
int crdt_orswot_read(crdt_ctx* ctx, const crdt_orswot_batch* batch, const crdt_read_queries* queries,
                     uint32_t n_actors, uint32_t flags, const crdt_read_out* out, void* stream);
int crdt_map_read_sizes(crdt_ctx* ctx, const crdt_map_read_view* view, const crdt_read_queries* queries,
                        size_t n_obj, uint32_t n_actors, const crdt_read_sizes* sizes, void* stream);
int crdt_map_read(crdt_ctx* ctx, const crdt_map_read_view* view, const crdt_read_queries* queries, size_t n_obj,
                  uint32_t n_actors, const crdt_read_out* out, void* stream);
int crdt_map_mvreg_get(crdt_ctx* ctx, const crdt_map_mvreg_slab* slab, const crdt_read_queries* queries,
                       size_t n_obj, uint32_t n_actors, uint32_t* d_out_n, uint64_t* d_out_clk,
                       uint64_t* d_out_val, uint32_t out_cap, void* stream);
int crdt_map_orswot_get_sizes(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, const crdt_read_queries* queries,
                              size_t n_obj, uint32_t n_actors, uint64_t* d_sizes, uint32_t* d_present, void* stream);
int crdt_map_orswot_get(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, const crdt_read_queries* queries,
                        size_t n_obj, uint32_t n_actors, uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes,
                        void* stream);
int crdt_map_map_get(crdt_ctx* ctx, const crdt_map_map_slab* slab, const crdt_read_queries* queries, size_t n_obj,
                     uint32_t n_actors, const crdt_map_mvreg_slab* out, uint32_t* d_present, void* stream);

/* ------------------------------------------------------------------------ *
 * Ingest / egest: the reference's binary form <-> canonical records
 * (SURVEY.md §8(f) rank 1). The reference form of an Orswot<M, A> is
 * `to_binary(&s)` = bincode 0.9 of its serde derives (src/lib.rs:62-83;
 * fields src/orswot.rs:26-30, src/vclock.rs:54-57): u64 little-endian
 * lengths before every map / set, fixed-width little-endian integers, HashMap
 * and HashSet elements in any order, BTreeMap keys ascending. Actors (A) and
 * members (M) are unsigned integers of actor_bytes / member_bytes in
 * {1, 2, 4, 8}; they are the record's actor ids / member keys as they stand.
 * Blob i is bytes [blob_off[i], blob_off[i] + blob_len[i]) of d_blobs
 * (blob_bytes long, any alignment).
 *
 * Ingest = from_binary + canonicalisation; a blob a record cannot hold
 * (zero counter, empty member clock / deferred clock / deferred set, actor
 * >= n_actors, duplicates, BTreeMap keys out of order, truncated or trailing
 * bytes) latches CRDT_ENONCANON; one with more than 16384 members or more
 * than 1024 deferred clocks latches CRDT_ECAPACITY, and so do the objects of
 * one call past its first 65536 with more than 256 members or 64 deferred
 * clocks (those are decoded by a second kernel from an HBM scratch). A blob's
 * length words are read front to back before anything else of it is looked
 * at, and the first that cannot be taken decides the code: a member or
 * deferred-clock count above the capacity is CRDT_ECAPACITY where it is read,
 * whatever the clocks before it hold and however few bytes follow it. 24 zero
 * bytes are valid (Orswot::default()). The other blobs of the call are
 * decoded as if the refused one were not there; of a refused blob nothing is
 * written outside the slot placed for it.
 *   1) crdt_orswot_bincode_record_sizes: d_sizes[i] = record bytes; 0 (and
 *      the code latched) for a blob whose length words are refused or that
 *      is not inside d_blobs. A blob that is bad only in what its fields hold
 *      (a zero counter, an actor >= n_actors or out of order, duplicates) is
 *      sized by its counts here and refused by crdt_orswot_from_bincode
 *      (the slot's contents are then unspecified)
 *      — or, without reading the blobs, crdt_orswot_bincode_record_bounds:
 *      d_bounds[i] >= the record bytes of any blob of length blob_len[i]
 *      (16-B multiple; <= 48 + 8 n_actors + blob_len * max(12/(wa+8),
 *      12/(wm+8), 8/wm)); records placed by bounds form a gapped batch, a
 *      valid input everywhere (crdt_orswot_compact removes the gaps)
 *   2) the caller places records (16-B aligned offsets, e.g. exclusive scan)
 *   3) crdt_orswot_from_bincode writes record i at d_out + d_out_off[i].
 * Egest = to_binary with HashMap / HashSet elements in ascending key (clock)
 * order — one of the orders the reference may produce, decoded to an equal
 * state by from_binary:
 *   1) crdt_orswot_bincode_sizes: d_sizes[i] = blob bytes
 *   2) the caller places blobs at 16-B aligned offsets (each zero-padded to 16)
 *   3) crdt_orswot_to_bincode writes them; a member key or an actor id that
 *      does not fit its byte width latches CRDT_ENONCANON (the blob's bytes
 *      are then unspecified), and so does the whole call, whatever its
 *      records hold, when n_actors - 1 does not fit actor_bytes.              */
int crdt_orswot_bincode_record_sizes(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes,
                                     const uint64_t* d_blob_off, const uint64_t* d_blob_len, size_t n_obj,
                                     uint32_t actor_bytes, uint32_t member_bytes, uint32_t n_actors,
                                     uint32_t flags, uint64_t* d_sizes, void* stream);
int crdt_orswot_bincode_record_bounds(crdt_ctx* ctx, const uint64_t* d_blob_len, size_t n_obj,
                                      uint32_t actor_bytes, uint32_t member_bytes, uint32_t n_actors, uint32_t flags,
                                      uint64_t* d_bounds, void* stream);
int crdt_orswot_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes,
                             const uint64_t* d_blob_off, const uint64_t* d_blob_len, size_t n_obj,
                             uint32_t actor_bytes, uint32_t member_bytes, uint32_t n_actors, uint32_t flags,
                             uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes, void* stream);
int crdt_orswot_bincode_sizes(crdt_ctx* ctx, const crdt_orswot_batch* batch, uint32_t n_actors,
                              uint32_t flags, uint32_t actor_bytes, uint32_t member_bytes, uint64_t* d_sizes,
                              void* stream);
int crdt_orswot_to_bincode(crdt_ctx* ctx, const crdt_orswot_batch* batch, uint32_t n_actors, uint32_t flags,
                           uint32_t actor_bytes, uint32_t member_bytes, uint8_t* d_out,
                           const uint64_t* d_out_off, size_t out_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Ingest / egest of MVReg<V, A> (src/mvreg.rs:42-46) and Map<K, MVReg<V, A>,
 * A> (src/map.rs:81-99; Entry :69-77): `to_binary` blobs (src/lib.rs:62-83)
 * <-> the slabs of crdt_mvreg_merge / crdt_map_mvreg_merge. bincode 0.9 of
 * the serde derives: a struct is its fields in order, a Vec / map / set a u64
 * little-endian length and its elements, integers fixed-width little-endian:
 *   VClock  u64 n | n x (A actor | u64 counter)           actors ascending
 *   MVReg   u64 n_vals | n_vals x (VClock | V val)        Vec order (state)
 *   Map     VClock clock
 *           u64 n_entries | n_entries x (K key | VClock entry clock | MVReg)
 *                                                         keys ascending
 *           u64 n_def | n_def x (VClock | u64 n | n x K)  HashMap: clocks in
 *                                        any order; BTreeSet: keys ascending
 * A, K and V are unsigned integers of actor_bytes / key_bytes / val_bytes in
 * {1, 2, 4, 8}, taken as the slab's actor ids, keys and values as they
 * stand. Blob i is bytes [blob_off[i], blob_off[i] + blob_len[i]) of d_blobs
 * (blob_bytes long; buffer and blobs at any alignment). All arrays are
 * device arrays.
 *
 * Ingest = from_binary + the slab's canonical form: keys ascending and
 * values in Vec order as in the blob, deferred clocks sorted into CLOCK ORDER
 * (the one thing ingest reorders), their key sets ascending as in the blob.
 * crdt_map_mvreg_from_bincode writes only the used slots of `out`;
 * crdt_mvreg_from_bincode zero-fills every unused slot of its object.
 * Latched per object (crdt_ctx_status; the other objects are unaffected, the
 * object's row is unspecified; the MVReg slab's count of that object is 0):
 *   CRDT_ENONCANON  a zero counter (a dense row cannot tell it from absent);
 *                   an actor >= n_actors; actors, keys or deferred-set keys
 *                   not strictly ascending; two equal deferred clocks; a blob
 *                   that ends early or has trailing bytes; a length word
 *                   larger than the bytes left could hold; a blob that is
 *                   not inside d_blobs. Every length word is checked against
 *                   the bytes left before anything it sizes is read: nothing
 *                   outside a blob's aligned 16-byte lines within d_blobs is
 *                   read.
 *   CRDT_ECAPACITY  a well-formed blob with more keys, values per register,
 *                   deferred clocks or deferred-set keys than out's
 *                   capacities.
 * Accepted, as the slab holds them: the empty map, an entry whose register
 * has no values, an empty entry / value / deferred clock (an all-zero row).
 *
 * Egest = to_binary with the deferred HashMap in the slab's CLOCK ORDER (one
 * of the orders the reference may produce; from_binary decodes an equal
 * state), in two calls:
 *   1) *_bincode_sizes: d_sizes[i] = blob bytes
 *   2) the caller places the blobs (any byte offsets, e.g. an exclusive scan)
 *   3) *_to_bincode writes blob i at d_out + d_out_off[i].
 * Latched per object: CRDT_ENONCANON for a count above its capacity or a key,
 * value or actor id that does not fit its byte width — that object's size is
 * 0 and nothing of it is written; CRDT_ECAPACITY for a blob placed past
 * out_bytes (not written).
 *
 * CRDT_EINVAL (before any device work): a null ctx or slab struct; a null
 * array with n_obj > 0; a width outside {1, 2, 4, 8}; n_actors == 0 (Map:
 * or > 128); ingest capacities outside the merges' per-side limits (Map:
 * kcap <= 4096, mcap <= 128, dcap <= 64, scap <= 4096; MVReg: out_cap <=
 * 1024), egest capacities outside those of a merge's output (twice them), a
 * zero capacity; out_bytes below the smallest blob (Map 24, MVReg 8) with
 * n_obj > 0. n_obj == 0 is CRDT_OK and launches nothing. CRDT_ENODEV without
 * a device (crdt_ctx_create).                                              */
int crdt_mvreg_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes,
                            const uint64_t* d_blob_off, const uint64_t* d_blob_len, size_t n_obj,
                            uint32_t actor_bytes, uint32_t val_bytes, uint32_t n_actors, uint32_t* d_out_n,
                            uint64_t* d_out_clk, uint64_t* d_out_val, uint32_t out_cap, void* stream);
int crdt_mvreg_bincode_sizes(crdt_ctx* ctx, const uint32_t* d_n, const uint64_t* d_clk, const uint64_t* d_val,
                             uint32_t cap, size_t n_obj, uint32_t n_actors, uint32_t actor_bytes,
                             uint32_t val_bytes, uint64_t* d_sizes, void* stream);
int crdt_mvreg_to_bincode(crdt_ctx* ctx, const uint32_t* d_n, const uint64_t* d_clk, const uint64_t* d_val,
                          uint32_t cap, size_t n_obj, uint32_t n_actors, uint32_t actor_bytes, uint32_t val_bytes,
                          uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes, void* stream);
int crdt_map_mvreg_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes,
                                const uint64_t* d_blob_off, const uint64_t* d_blob_len, size_t n_obj,
                                uint32_t actor_bytes, uint32_t key_bytes, uint32_t val_bytes, uint32_t n_actors,
                                const crdt_map_mvreg_slab* out, void* stream);
int crdt_map_mvreg_bincode_sizes(crdt_ctx* ctx, const crdt_map_mvreg_slab* slab, size_t n_obj, uint32_t n_actors,
                                 uint32_t actor_bytes, uint32_t key_bytes, uint32_t val_bytes, uint64_t* d_sizes,
                                 void* stream);
int crdt_map_mvreg_to_bincode(crdt_ctx* ctx, const crdt_map_mvreg_slab* slab, size_t n_obj, uint32_t n_actors,
                              uint32_t actor_bytes, uint32_t key_bytes, uint32_t val_bytes, uint8_t* d_out,
                              const uint64_t* d_out_off, size_t out_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Ingest / egest of the two Map types whose values are containers:
 * Map<K, Orswot<M, A>, A> <-> crdt_map_orswot_slab and Map<K, Map<K2,
 * MVReg<V, A>, A>, A> (the reference's TestMap, test/map.rs:4-8) <->
 * crdt_map_map_slab. The format is the one above, with
 *   Orswot  VClock clock                                  src/orswot.rs:26-30
 *           u64 n_mem | n_mem x (M member | VClock)       HashMap: any order
 *           u64 n_def | n_def x (VClock | u64 n | n x M)  HashMap of HashSet:
 *                                  clocks in any order, members in any order
 *   Map<K, V>  as above with an entry = K key | VClock entry clock | V, where
 *           V = Orswot<M, A> (crdt_map_orswot_*) or V = Map<K2, MVReg<V2, A>,
 *           A>, the Map form again (crdt_map_map_*).
 * Widths (actor, key, member / inner key, value bytes) are in {1, 2, 4, 8};
 * blobs, offsets, lengths, the stream and the two-call egest are as for
 * crdt_map_mvreg_*. Inner map k of object i is row i * kcap + k of out->inner.
 *
 * Ingest = from_binary + the slab's canonical form; only the used slots of
 * `out` are written. Map<K, Orswot>: every nested set's members are sorted
 * ascending (each member clock row follows its member), its deferred clocks
 * put into CLOCK ORDER, each deferred member set sorted ascending, and the
 * map's deferred clocks put into CLOCK ORDER. The nested map: the outer and
 * the inner deferred clocks are put into CLOCK ORDER; everything else is a
 * BTree (checked strictly ascending) or a Vec (order kept). Accepted: the
 * empty map, an empty nested set or inner map, an empty clock anywhere (an
 * empty member clock is an all-zero row), a register without values.
 * Latched per object, the other objects unaffected:
 *   CRDT_ENONCANON  as for crdt_map_mvreg_from_bincode, and: two equal
 *                   members in one nested set or in one deferred member set.
 *   CRDT_ECAPACITY  a well-formed blob with more of anything than out's
 *                   capacities.
 * Egest writes every unordered container in the slab's order; errors as for
 * crdt_map_mvreg_to_bincode (a count above its capacity, or a key, member,
 * value or actor id that does not fit its width: CRDT_ENONCANON, size 0,
 * nothing written; a blob placed past out_bytes: CRDT_ECAPACITY).
 *
 * CRDT_EINVAL (before any device work): a null ctx or slab struct; a null
 * array with n_obj > 0; a width outside {1, 2, 4, 8}; n_actors == 0 or > 128;
 * a zero capacity; ingest capacities outside the merges' static per-side
 * limits (Map<K, Orswot>: kcap <= 4096, mcap, vdcap, vscap, dcap <= 256, scap
 * <= 4096 — the merge's 64 KB workspace rule is the merge's own and is not
 * applied; nested map: outer kcap <= 4096, dcap <= 64, scap <= 4096, inner
 * as crdt_map_mvreg_merge's); egest capacities above twice those; out_bytes
 * below 24 with n_obj > 0. n_obj == 0 is CRDT_OK and launches nothing.      */
int crdt_map_orswot_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes,
                                 const uint64_t* d_blob_off, const uint64_t* d_blob_len, size_t n_obj,
                                 uint32_t actor_bytes, uint32_t key_bytes, uint32_t member_bytes, uint32_t n_actors,
                                 const crdt_map_orswot_slab* out, void* stream);
int crdt_map_orswot_bincode_sizes(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, size_t n_obj, uint32_t n_actors,
                                  uint32_t actor_bytes, uint32_t key_bytes, uint32_t member_bytes, uint64_t* d_sizes,
                                  void* stream);
int crdt_map_orswot_to_bincode(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, size_t n_obj, uint32_t n_actors,
                               uint32_t actor_bytes, uint32_t key_bytes, uint32_t member_bytes, uint8_t* d_out,
                               const uint64_t* d_out_off, size_t out_bytes, void* stream);
int crdt_map_map_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                              const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t key_bytes,
                              uint32_t inner_key_bytes, uint32_t val_bytes, uint32_t n_actors,
                              const crdt_map_map_slab* out, void* stream);
int crdt_map_map_bincode_sizes(crdt_ctx* ctx, const crdt_map_map_slab* slab, size_t n_obj, uint32_t n_actors,
                               uint32_t actor_bytes, uint32_t key_bytes, uint32_t inner_key_bytes, uint32_t val_bytes,
                               uint64_t* d_sizes, void* stream);
int crdt_map_map_to_bincode(crdt_ctx* ctx, const crdt_map_map_slab* slab, size_t n_obj, uint32_t n_actors,
                            uint32_t actor_bytes, uint32_t key_bytes, uint32_t inner_key_bytes, uint32_t val_bytes,
                            uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * LWWReg<u64, M>, batched (lwwreg.hip): FunkyCvRDT::merge, FunkyCmRDT::apply,
 * update, a rank-order fold and the bincode codec. Reference: src/lwwreg.rs
 * :27-32 (state), :56-66 (merge), :69-77 (apply), :104-118 (update).
 *
 * Layout, all device arrays, structure-of-arrays:
 *   val[n]                    u64: the caller's interned value key, bijective
 *                             as for MVReg values (key equality is value
 *                             equality);
 *   marker[n][marker_words]   u64, row-major, marker_words 1 or 2. Markers
 *                             compare lexicographically, word 0 first (Rust
 *                             tuple Ord; test/lwwreg.rs:39-45 uses a 2-tuple).
 *
 * merge(self, other) (src/lwwreg.rs:56-66):
 *   other.marker > self.marker                  self := other, Ok;
 *   markers equal and values differ             self unchanged, Err
 *                                               (ConflictingMarker);
 *   otherwise (equal marker and value included) self unchanged, Ok.
 * update(val, marker) (:104-118) and apply(op) (:74-76) are the same rule as
 * merging LWWReg{val, marker}: one device function serves all three.
 *
 * A list of ops o_1..o_k on state o_0 has the sequential meaning: an erring op
 * changes nothing, later ops still apply, every op's Result is reported. In
 * closed form the final state is the first element of o_0..o_k attaining the
 * largest marker, and op i errs iff its marker equals the largest marker of
 * o_0..o_{i-1} and its value differs from that of the first element attaining
 * it (an exclusive prefix scan with a (+) b = b.marker > a.marker ? b : a).
 *
 * CONFLICTS ARE RESULTS, NOT FAULTS: an Err of the reference is reported in
 * the call's own outputs (bitmap, counts, per-op bytes) and is never latched
 * on the context: crdt_ctx_status stays CRDT_OK after a batch full of
 * conflicts. Only malformed input (an obj_end out of order, a value too wide
 * for its bincode width) latches.
 *
 * Every call: CRDT_EINVAL (before any device work) for a null ctx, a null
 * required array with n > 0, a null ops struct, a null op array whose count
 * says it is non-empty, marker_words outside {1, 2}, a byte width outside
 * {1, 2, 4, 8}, n_reps of 0 or above 32, a null view pointer, and an output
 * pointer equal to an input it must not alias (self equal to other in merge,
 * out equal to a replica other than replica 0 in fold, an op array equal to a
 * state array in apply, blobs equal to a state array in the codec).
 * Otherwise n == 0 is CRDT_OK, launches nothing and writes nothing, null
 * arrays included.
 *
 * crdt_lwwreg_merge: self[i].merge(other[i]), in place on self.
 *   d_conflict   u64[(n + 63) / 64], nullable: bit i % 64 of word i / 64 is set
 *                iff register i's merge returned Err. Every word is written,
 *                tail bits are zero.
 *   d_n_conflict one u64, nullable: overwritten with the number of conflicts.
 *   Both may be null. 16-byte aligned arrays take 16-byte loads and stores.
 *
 * crdt_lwwreg_apply: register i applies ops [obj_end[i-1], obj_end[i]) in
 * order, in place (the obj_end convention of crdt_clock_ops).
 *   d_n_err[i]   u32, required: the number of register i's ops that returned
 *                Err; written for every i, 0 for an empty list.
 *   d_op_err[j]  u8, nullable: op j's Result, 0 Ok, 1 Err.
 *   An object whose range decreases or runs past n_ops latches
 *   CRDT_ENONCANON: it is left untouched with d_n_err[i] = 0 (its ops' bytes
 *   of d_op_err are not written), the other objects apply; nothing outside
 *   the op arrays is read. Lists shorter than CRDT_LWWREG_WAVE_MIN_OPS are
 *   applied by one lane each, longer ones by a wave in chunks of 64 ops.
 *
 * crdt_lwwreg_fold: out[i] = reps[0][i].merge(reps[1][i]).merge(reps[2][i])...
 * in rank order (the fixed-order convention of crdt_orswot_fold), one pass:
 * every replica's state is read once, the output written once. h_reps is a
 * HOST array of n_reps views, 1 <= n_reps <= 32. d_n_err[i] (u32, nullable)
 * counts the erring merges of register i. The output may be replica 0's
 * arrays (in place), never another replica's.
 *
 * crdt_lwwreg_from_bincode / crdt_lwwreg_to_bincode: to_binary of
 * LWWReg<V, M> is the struct's fields in order (src/lwwreg.rs:27-32): val,
 * then the marker words, each fixed-width little-endian. So a blob has the
 * constant size val_bytes + marker_bytes0 (+ marker_bytes1 with two marker
 * words; ignored with one) and no sizes call exists. Blob i is at d_blobs +
 * i * stride, at any alignment; stride below the blob size is CRDT_EINVAL.
 * Ingest widens to u64. Egest narrows: a value or marker word that does not
 * fit its width latches CRDT_ENONCANON, that blob is not written, the others
 * are. Bytes between a blob's end and the next stride are never touched.
 * ------------------------------------------------------------------------ */
#define CRDT_LWWREG_WAVE_MIN_OPS 16  /* shortest op list the wave-per-register form of crdt_lwwreg_apply takes */
#define CRDT_LWWREG_MAX_REPS 32
typedef struct crdt_lwwreg_ops {   /* all device arrays */
  const uint64_t* obj_end;  /* n_obj: register i's ops are [obj_end[i-1], obj_end[i]) */
  const uint64_t* val;      /* n_ops */
  const uint64_t* marker;   /* n_ops x marker_words */
  size_t n_ops;
} crdt_lwwreg_ops;
typedef struct crdt_lwwreg_view {  /* one replica's registers, device arrays */
  const uint64_t* val;
  const uint64_t* marker;
} crdt_lwwreg_view;
int crdt_lwwreg_merge(crdt_ctx* ctx, uint64_t* d_self_val, uint64_t* d_self_marker, const uint64_t* d_other_val,
                      const uint64_t* d_other_marker, size_t n, uint32_t marker_words, uint64_t* d_conflict,
                      uint64_t* d_n_conflict, void* stream);
int crdt_lwwreg_apply(crdt_ctx* ctx, uint64_t* d_self_val, uint64_t* d_self_marker, const crdt_lwwreg_ops* ops,
                      size_t n_obj, uint32_t marker_words, uint32_t* d_n_err, uint8_t* d_op_err, void* stream);
int crdt_lwwreg_fold(crdt_ctx* ctx, const crdt_lwwreg_view* h_reps, uint32_t n_reps, size_t n, uint32_t marker_words,
                     uint64_t* d_out_val, uint64_t* d_out_marker, uint32_t* d_n_err, void* stream);
int crdt_lwwreg_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t stride, size_t n, uint32_t val_bytes,
                             uint32_t marker_words, uint32_t marker_bytes0, uint32_t marker_bytes1,
                             uint64_t* d_out_val, uint64_t* d_out_marker, void* stream);
int crdt_lwwreg_to_bincode(crdt_ctx* ctx, const uint64_t* d_val, const uint64_t* d_marker, size_t n,
                           uint32_t val_bytes, uint32_t marker_words, uint32_t marker_bytes0, uint32_t marker_bytes1,
                           uint8_t* d_blobs, size_t stride, void* stream);

/* ------------------------------------------------------------------------ *
 * bincode of the clocks, the counters and their ops (clock_bincode.hip):
 * `to_binary` / `from_binary` (src/lib.rs:62-83) of VClock, GCounter and
 * PNCounter states, on dense rows and on CSR runs, and of their CmRDT ops.
 *
 * Wire format (bincode 0.9 of the serde derives; A = an unsigned integer of
 * actor_bytes in {1, 2, 4, 8}, little-endian, taken as the interned actor id):
 *   VClock<A>     u64 n | n x (A actor | u64 counter), actors strictly
 *                 ascending (a BTreeMap, src/vclock.rs:53-57)
 *   GCounter<A>   its `inner` VClock (src/gcounter.rs:26-28): the same bytes
 *   PNCounter<A>  VClock p | VClock n (src/pncounter.rs:33-36)
 *   Dot<A>        A actor | u64 counter (src/vclock.rs:33-39): the Op of
 *                 VClock and GCounter, actor_bytes + 8 bytes
 *   PNCounter Op  Dot | u32 variant index of Dir, Pos = 0, Neg = 1
 *                 (src/pncounter.rs:39-56): actor_bytes + 12 bytes
 * BTreeMap order makes the bytes of a state unique: ingest reorders nothing
 * and egest has one answer. (The reference's tests assert no bytes: parity
 * unpinned by reference output.)
 *
 * State blob i is [d_blob_off[i], d_blob_off[i] + d_blob_len[i]) of d_blobs,
 * at any alignment. n_clocks is 1 for VClock / GCounter, 2 for PNCounter.
 * Nothing outside a blob's aligned 16-byte lines within d_blobs is read.
 *
 * Dense rows (the layout of crdt_vclock_dense_merge; PNCounter: the [P|N] row
 * of 2 * n_actors slots):
 *   crdt_clock_dense_from_bincode writes every slot of every row (absent
 *     actors 0; each row leaves the chip once, in full-width stores).
 *   crdt_clock_dense_bincode_sizes: d_sizes[i] = 8 * n_clocks + (nonzero
 *     slots of row i) * (actor_bytes + 8).
 *   crdt_clock_dense_to_bincode writes blob i at d_out + d_out_off[i], any
 *     byte offset (the caller places the blobs, e.g. by an exclusive scan of
 *     the sizes); no byte outside the blobs is written.
 * CSR runs (crdt_clock_csr / crdt_clock_csr_out; PNCounter: two batches as in
 * crdt_pncounter_csr_merge; the _n arguments are null when n_clocks == 1):
 *   crdt_clock_csr_bincode_lens: the entry counts of every blob, from its
 *     framing alone (each length word against the bytes left, and the exact
 *     blob length); a blob with bad framing gets 0 and is latched.
 *   crdt_clock_csr_from_bincode: HERE out.off IS AN INPUT — the caller places
 *     the runs (e.g. an exclusive scan of the lens; gaps are fine); out.len
 *     and the entries are written. A run placed past out.n_entries latches
 *     CRDT_ECAPACITY (len 0). The output is a valid (gapped) input batch of
 *     every crdt_*_csr_* call when the caller's offsets ascend.
 *   crdt_clock_csr_bincode_sizes / crdt_clock_csr_to_bincode: as the dense
 *     pair; self_n null selects one clock per object.
 * Ops: fixed-size blobs, op j at d_blobs + j * stride, at any alignment (as
 * in the LWWReg codec); with_dir != 0 selects the PNCounter Op.
 *   crdt_clock_ops_from_bincode fills the actor / counter / dir arrays of a
 *     crdt_clock_ops (obj_end stays the caller's: grouping is not on the
 *     wire); d_dir is not touched without with_dir.
 *   crdt_clock_ops_to_bincode: bytes between a blob's end and the next
 *     stride are never touched.
 *
 * Latched per object (crdt_ctx_status), the other objects unaffected:
 *   CRDT_ENONCANON on ingest: a zero counter; actors not strictly ascending
 *     (or duplicated); an actor >= n_actors (dense) or >= 2^32 (CSR, ops); a
 *     blob that ends early or has trailing bytes; a length word larger than
 *     the bytes left can hold (checked before any multiply) or than any
 *     canonical clock; a blob not inside d_blobs; a PNCounter whose p runs to
 *     or past the blob's end; an op whose Dir index is above 1 (all four
 *     bytes are compared). A bad dense object's row is all zero, a bad CSR
 *     object has len 0 (both clocks of a PNCounter), a bad op becomes actor
 *     0xFFFFFFFF, counter 0, dir 0, which every apply skips and latches.
 *   CRDT_ENONCANON on egest (size 0, nothing written): an actor id with a
 *     non-zero counter that does not fit actor_bytes; a CSR run that is not
 *     canonical (actors not strictly ascending, a zero counter) or lies
 *     outside [0, n_entries); an op dir above 1.
 *   CRDT_ECAPACITY on egest: a blob placed past out_bytes (not written).
 * CRDT_EINVAL (before any device work): a null ctx; a null array (or struct)
 * with a non-zero count; a width outside {1, 2, 4, 8}; n_actors == 0;
 * n_clocks outside {1, 2}; self_n->n_obj != self_p->n_obj; a stride below
 * the op size; an output array equal to an input array. Otherwise zero
 * objects / ops is CRDT_OK and launches nothing. Clocks of any length.
 * ------------------------------------------------------------------------ */
int crdt_clock_dense_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                                  const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t n_actors,
                                  uint32_t n_clocks, uint64_t* d_rows, void* stream);
int crdt_clock_dense_bincode_sizes(crdt_ctx* ctx, const uint64_t* d_rows, size_t n_obj, uint32_t n_actors,
                                   uint32_t n_clocks, uint32_t actor_bytes, uint64_t* d_sizes, void* stream);
int crdt_clock_dense_to_bincode(crdt_ctx* ctx, const uint64_t* d_rows, size_t n_obj, uint32_t n_actors,
                                uint32_t n_clocks, uint32_t actor_bytes, uint8_t* d_out, const uint64_t* d_out_off,
                                size_t out_bytes, void* stream);
int crdt_clock_csr_bincode_lens(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                                const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t n_clocks,
                                uint32_t* d_len_p, uint32_t* d_len_n, void* stream);
int crdt_clock_csr_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                                const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t n_clocks,
                                const crdt_clock_csr_out* out_p, const crdt_clock_csr_out* out_n, void* stream);
int crdt_clock_csr_bincode_sizes(crdt_ctx* ctx, const crdt_clock_csr* self_p, const crdt_clock_csr* self_n,
                                 uint32_t actor_bytes, uint64_t* d_sizes, void* stream);
int crdt_clock_csr_to_bincode(crdt_ctx* ctx, const crdt_clock_csr* self_p, const crdt_clock_csr* self_n,
                              uint32_t actor_bytes, uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes,
                              void* stream);
int crdt_clock_ops_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t stride, size_t n_ops,
                                uint32_t actor_bytes, uint32_t with_dir, uint32_t* d_actor, uint64_t* d_counter,
                                uint32_t* d_dir, void* stream);
int crdt_clock_ops_to_bincode(crdt_ctx* ctx, const uint32_t* d_actor, const uint64_t* d_counter,
                              const uint32_t* d_dir, size_t n_ops, uint32_t actor_bytes, uint32_t with_dir,
                              uint8_t* d_blobs, size_t stride, void* stream);

/* ------------------------------------------------------------------------ *
 * bincode of the Orswot, MVReg and Map ops (ops_bincode.hip): the wire form of
 * the `Op` enums replicas exchange (all derive Serialize / Deserialize:
 * src/orswot.rs:36-53, src/mvreg.rs:49-59, src/map.rs:102-123), into and out
 * of the arrays of crdt_orswot_ops, crdt_mvreg_ops, crdt_map_mvreg_ops,
 * crdt_map_orswot_ops and crdt_map_map_ops. One family of four calls serves
 * the five op types, selected by op_type. obj_end is not on the wire: grouping
 * stays the caller's, as in crdt_clock_ops_from_bincode.
 *
 * Wire format (bincode 0.9 of the serde derives): an enum is a little-endian
 * u32 variant index followed by its fields in declaration order; a VClock is
 * u64 n | n x (A actor | u64 counter), actors strictly ascending. A, K, M / K2
 * and V are unsigned little-endian integers of actor_bytes, key_bytes,
 * key2_bytes and val_bytes, each in {1, 2, 4, 8}; a width is read only where
 * the op type has the field.
 *   Orswot Op  Add: 0 | A actor | u64 counter | M member    Rm: 1 | VClock | M member   (M = key2)
 *   MVReg  Op  Put: 0 | VClock | V val
 *   Map    Op  Nop: 0     Rm: 1 | VClock | K key     Up: 2 | A actor | u64 counter | K key | <V::Op>
 *     V = MVReg            <V::Op> = Put                                kind CRDT_MAP_OP_UP 2
 *     V = Orswot           <V::Op> = Add -> kind CRDT_MAP_OP_UP 2,  Rm -> CRDT_MAP_OP_UP_RM 3
 *     V = Map<K2, MVReg>   <V::Op> = Nop -> CRDT_MAPMAP_OP_UP_NOP 4,  Rm { clock, key2 } -> UP_RM 3,
 *                                    Up { dot2, key2, Put } -> UP_UP 2 (actor2 / counter2 / key2 / val)
 *   e.g. Orswot Add { dot (3, 5), member 9 } at actor_bytes 1, key2_bytes 2 is the 15 bytes
 *     00000000 03 0500000000000000 0900; the nested Up { (1, 7), key 10, Up { (2, 3), key2 11,
 *     Put { {1: 7}, 42 } } } at all widths 1 is the 50 bytes 02000000 01 0700000000000000 0A
 *     02000000 02 0300000000000000 0B 00000000 0100000000000000 01 0700000000000000 2A.
 * crdt_map_orswot_ops holds one dot per op: the nested Add's dot is the Up's,
 * as Map::update builds it. Ingest latches CRDT_ENONCANON for a blob whose
 * two dots differ; egest writes the dot twice. (The reference's tests assert
 * no bytes: parity unpinned by reference output.)
 *
 * Op j is the blob [d_blob_off[j], d_blob_off[j] + d_blob_len[j]) of d_blobs,
 * at any alignment. Nothing outside a blob's aligned 16-byte lines within
 * d_blobs is read.
 *
 * Ingest is two calls with the caller's scan between them:
 *   crdt_ops_bincode_clk_lens: d_clk_len[j] = the clock pairs of op j, from
 *     its framing alone (the variant indices, the clock's length word against
 *     the bytes left before any multiply, the exact blob length, the blob
 *     inside d_blobs); 0 for Add, Nop and UP_NOP. A badly framed op gets 0
 *     pairs (CRDT_OPS_MVREG: 1, for the sentinel below) and is latched.
 *   The caller takes the inclusive prefix sum of the lens into clk_end.
 *   crdt_ops_from_bincode: HERE out->clk_end IS AN INPUT. Every array the op
 *     type uses is written (fields an op's kind does not carry: 0) and op j's
 *     pairs at [clk_end[j-1], clk_end[j]). A span that is not the op's length
 *     or that leaves [0, n_clk) latches CRDT_ECAPACITY for that op.
 *   A bad op is latched per op, the other ops unaffected: it comes out as kind
 *     CRDT_OP_KIND_BAD with every other field 0 (every apply rejects an
 *     unknown kind with CRDT_ENONCANON); CRDT_OPS_MVREG has no kind array:
 *     there the first pair of the op's span, if it has one, is (0xFFFFFFFF,
 *     0), which crdt_mvreg_apply rejects. The other pairs of a bad op's span
 *     are unspecified. d_op_err[j], when given, is 0 or the op's CRDT_E* code.
 *   CRDT_ENONCANON on ingest: a blob that ends early, has trailing bytes or is
 *     shorter than its variant word; a variant index above the type's last,
 *     outer or inner (all four bytes are compared); a length word larger than
 *     the bytes left can hold; clock actors not strictly ascending; a zero
 *     counter in a clock; an actor >= 2^32 in a clock or in a dot; the
 *     Map<Orswot> dot mismatch; a blob not inside d_blobs (off + len wrapping
 *     included). A dot with counter 0 is accepted (the applies treat it as a
 *     duplicate); actor ranges are the applies' to check; clocks of any length.
 * Egest: crdt_ops_bincode_sizes, the caller's placement at any byte offsets,
 *   crdt_ops_to_bincode. Per op CRDT_ENONCANON (size 0, nothing written): an
 *   unknown kind; a key, member, value or actor that does not fit its width;
 *   an op clock that is not canonical; pairs owned by a kind that carries no
 *   clock (the wire cannot say it); clk_end decreasing or past n_clk. A blob
 *   placed past out_bytes latches CRDT_ECAPACITY and is not written. No byte
 *   outside the blobs is written.
 * CRDT_EINVAL (before any device work): a null ctx, widths or arrays struct;
 * op_type > 4; a used width outside {1, 2, 4, 8}; a null array the type uses
 * (or a null d_blobs / d_blob_off / d_blob_len / d_clk_len / d_sizes / d_out /
 * d_out_off) with n_ops > 0; a null pair array with n_clk > 0; an output
 * array equal to an input array. n_ops == 0 is CRDT_OK and launches nothing.
 * ------------------------------------------------------------------------ */
#define CRDT_OPS_ORSWOT 0u     /* arrays of crdt_orswot_ops     */
#define CRDT_OPS_MVREG 1u      /* arrays of crdt_mvreg_ops      */
#define CRDT_OPS_MAP_MVREG 2u  /* arrays of crdt_map_mvreg_ops  */
#define CRDT_OPS_MAP_ORSWOT 3u /* arrays of crdt_map_orswot_ops */
#define CRDT_OPS_MAP_MAP 4u    /* arrays of crdt_map_map_ops    */
#define CRDT_OP_KIND_BAD 0xFFFFFFFFu
typedef struct crdt_op_widths {
  uint32_t actor_bytes, key_bytes, key2_bytes, val_bytes;
} crdt_op_widths;
typedef struct crdt_op_arrays { /* device; n_ops long unless said; null where the op type has no such field */
  uint32_t* kind;     /* all but MVREG */
  uint64_t* key;      /* the three Map types: the (outer) key */
  uint32_t* actor;    /* the (outer) dot: all but MVREG */
  uint64_t* counter;
  uint64_t* key2;     /* ORSWOT, MAP_ORSWOT: member; MAP_MAP: the inner key */
  uint32_t* actor2;   /* MAP_MAP: the inner dot */
  uint64_t* counter2;
  uint64_t* val;      /* MVREG, MAP_MVREG, MAP_MAP: the Put's value */
  uint64_t* clk_end;  /* n_ops; AN INPUT of crdt_ops_from_bincode */
  uint32_t* clk_act;  /* n_clk */
  uint64_t* clk_ctr;  /* n_clk */
  size_t n_ops, n_clk;
} crdt_op_arrays;
int crdt_ops_bincode_clk_lens(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                              const uint64_t* d_blob_len, size_t n_ops, uint32_t op_type, const crdt_op_widths* widths,
                              uint32_t* d_clk_len, void* stream);
int crdt_ops_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                          const uint64_t* d_blob_len, uint32_t op_type, const crdt_op_widths* widths,
                          const crdt_op_arrays* out, uint32_t* d_op_err, void* stream);
int crdt_ops_bincode_sizes(crdt_ctx* ctx, uint32_t op_type, const crdt_op_widths* widths, const crdt_op_arrays* ops,
                           uint64_t* d_sizes, void* stream);
int crdt_ops_to_bincode(crdt_ctx* ctx, uint32_t op_type, const crdt_op_widths* widths, const crdt_op_arrays* ops,
                        uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes, void* stream);

/* Dense synthetic counters: u64[n_obj][n_actors] rows for objects
 * [first_obj, first_obj+n_obj), counter U[0, 2^bits) with `pct_zero` % zeros. */
int crdt_dense_generate(uint64_t seed, size_t first_obj, size_t n_obj, uint32_t n_actors,
                        uint32_t bits, uint32_t pct_zero, int n_threads, uint64_t* h_rows);

/* Causal::truncate, batched (src/orswot.rs:159-172; the Map of Orswots calls it
 * on every value it keeps, src/map.rs): out[i] := self[i] after
 * self[i].truncate(&clock[i]) — merge with an empty Orswot whose clock is
 * clock[i] (incl. apply_deferred), then clock[i] subtracted from the top clock
 * and from every member clock. clocks: a crdt_clock_csr batch of the same
 * n_obj (any clock form of the records: actor ids as in the records).
 * flags: 0 or CRDT_ORSWOT_SPARSE_CLOCK (the batch's record form). A truncated
 * record is never larger than its input: record i is written at
 * d_out_off[i] := self.off[i] (set by the call), so out_bytes >= self.bytes
 * suffices. A member whose clock the subtract empties is kept with an empty
 * clock, as in the reference, and its record carries
 * CRDT_ORSWOT_EMPTY_MEMBER_CLOCK; such a record is a valid input of this call
 * (truncating it again drops those members: empty <= c, src/orswot.rs:98-103).
 * A malformed record or clock run (actors not strictly increasing, a zero
 * counter) latches CRDT_ENONCANON (that record is not written). d_out must
 * not overlap the input records (CRDT_EINVAL): the call is not in place. */
int crdt_orswot_truncate(crdt_ctx* ctx, const crdt_orswot_batch* self, const crdt_clock_csr* clocks,
                         uint32_t n_actors, uint32_t flags, uint8_t* d_out, uint64_t* d_out_off, size_t out_bytes,
                         void* stream);

/* Host op-path builder used to construct states (tests, KAT scripts): an
 * opaque host Orswot with the reference's op semantics (src/orswot.rs:61-85,
 * 195-211, 235-243), encoded to / decoded from canonical records. */
typedef struct crdt_host_orswot crdt_host_orswot;
crdt_host_orswot* crdt_host_orswot_new(void);
crdt_host_orswot* crdt_host_orswot_clone(const crdt_host_orswot* o);
void crdt_host_orswot_free(crdt_host_orswot* o);
/* Op::Add { dot: (actor, counter), member }  (src/orswot.rs:66-79) */
int crdt_host_orswot_apply_add(crdt_host_orswot* o, uint32_t actor, uint64_t counter,
                               uint64_t member);
/* Op::Rm { clock, member }  (src/orswot.rs:80-82) — clock as sorted runs */
int crdt_host_orswot_apply_rm(crdt_host_orswot* o, uint64_t member, const uint32_t* actors,
                              const uint64_t* counters, uint32_t n);
/* Encode into h_rec (capacity cap); returns bytes written or a negative code. */
long crdt_host_orswot_encode(const crdt_host_orswot* o, uint32_t n_actors, uint8_t* h_rec,
                             size_t cap);
/* flags: 0 (dense, n_actors slots) or CRDT_ORSWOT_SPARSE_CLOCK (CSR top clock). */
long crdt_host_orswot_encode_ex(const crdt_host_orswot* o, uint32_t n_actors, uint32_t flags,
                                uint8_t* h_rec, size_t cap);
crdt_host_orswot* crdt_host_orswot_decode(const uint8_t* h_rec, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* CRDTS_HIP_H */
