// Internal launch entry points (the C ABI in api.hip validates and calls these).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crdts_hip.h"

namespace crdts_hip {

// The join launches' sequence on one context (its control-word set
// alternates per launch; dirty: zero both sets before the next launch).
struct JoinSeq {
  uint32_t seq;
  bool dirty;
};
int launch_orswot_merge(const uint8_t* Lb, const uint64_t* Loff, uint64_t Lbytes, const uint8_t* Rb,
                        const uint64_t* Roff, uint64_t Rbytes, uint8_t* Ob, uint64_t* Ooff,
                        uint64_t Obytes, uint64_t n_obj, uint32_t n_actors, int* status, uint32_t* ctl,
                        uint64_t* list, uint32_t list_cap, hipStream_t stream, int blocks_per_cu,
                        int variant, JoinSeq* js);

int launch_orswot_merge_sparse(const uint8_t* Lb, const uint64_t* Loff, uint64_t Lbytes, const uint8_t* Rb,
                               const uint64_t* Roff, uint64_t Rbytes, uint8_t* Ob, uint64_t* Ooff, uint64_t Obytes,
                               uint64_t n_obj, uint32_t n_actors, int* status, uint32_t* ctl, uint64_t* list,
                               uint32_t list_cap, hipStream_t stream, int sparse_variant, JoinSeq* js);

// Sparse clock joins: n_jobs (1 or 2: PNCounter's P and N) batches in one launch.
int launch_clock_csr_merge(const crdt_clock_csr* const* self, const crdt_clock_csr* const* other,
                           const crdt_clock_csr_out* const* out, int n_jobs, int* status, hipStream_t stream);

// Clock fold (clock_fold.hip): rows / reps are host arrays of 1 <= n_reps <=
// CRDT_CLOCK_FOLD_MAX_REPS device pointers / views of one n_obj (api.hip checks
// the rest); out may be one of rows; the CSR out is sized for the entries' sum.
int launch_clock_dense_fold(const uint64_t* const* rows, uint32_t n_reps, uint64_t* out, uint64_t n_words,
                            hipStream_t stream);
int launch_clock_csr_fold(const crdt_clock_csr* reps, uint32_t n_reps, const crdt_clock_csr_out& out, int* status,
                          hipStream_t stream);

int launch_orswot_truncate(const crdt_orswot_batch& self, const crdt_clock_csr& clocks, uint32_t A, uint32_t flags,
                           uint8_t* out, uint64_t* out_off, uint64_t out_bytes, int* status, uint32_t* ctl,
                           uint64_t* list, uint32_t list_cap, hipStream_t stream);

int launch_dense_max(uint64_t* self, const uint64_t* other, uint64_t n_words, hipStream_t stream);

// The clocks' op path (clock_ops.hip). Dense rows in place: the three binops
// flat over n_words like launch_dense_max; apply (pn: [P|N] rows and ops.dir)
// and get walk the op batch; value reduces rows of A (pn: 2 * A) slots.
enum { kClockTruncate = 0, kClockSubtract = 1, kClockIntersection = 2 };
int launch_dense_clock_binop(int op, uint64_t* self, const uint64_t* other, uint64_t n_words, hipStream_t stream);
int launch_dense_clock_apply(uint64_t* rows, const crdt_clock_ops& ops, bool pn, uint64_t n_obj, uint32_t A,
                             int* status, hipStream_t stream);
int launch_dense_clock_get(const uint64_t* rows, const crdt_clock_ops& queries, uint64_t* out, uint64_t n_obj,
                           uint32_t A, int* status, hipStream_t stream);
int launch_dense_clock_value(const uint64_t* rows, uint64_t* out, bool pn, uint64_t n_obj, uint32_t A,
                             hipStream_t stream);
// CSR runs, out != in: the filters place out at self's offsets, apply at
// self.off + obj_end[i-1]; apply's scratch holds clock_csr_apply_scratch_bytes
// (null only with no ops), 8-byte aligned.
int launch_clock_csr_filter(int op, const crdt_clock_csr& self, const crdt_clock_csr& other,
                            const crdt_clock_csr_out& out, int* status, hipStream_t stream);
size_t clock_csr_apply_scratch_bytes(const crdt_clock_ops& ops);
int launch_clock_csr_apply(const crdt_clock_csr& self, const crdt_clock_ops& ops, const crdt_clock_csr_out& out,
                           uint8_t* scratch, int* status, hipStream_t stream);
int launch_clock_csr_value(const crdt_clock_csr& self, uint64_t* out, int* status, hipStream_t stream);
int launch_clock_csr_get(const crdt_clock_csr& self, const crdt_clock_ops& queries, uint64_t* out, int* status,
                         hipStream_t stream);

int launch_orswot_validate(const uint8_t* base, const uint64_t* off, uint64_t bytes, uint64_t n_obj,
                           uint32_t n_actors, uint32_t flags, int* status, hipStream_t stream);

// Bounds-checked record sizes (size 0 + CRDT_ENONCANON latched for a record
// out of [0, bytes)), and the copy of sizes[i] bytes per record.
int launch_record_sizes(const uint8_t* base, const uint64_t* off, uint64_t bytes, uint64_t n_obj, uint64_t* sizes,
                        int* status, hipStream_t stream);
// records whose [dst_off, dst_off + size) does not fit dst_bytes are not copied
int launch_record_copy(const uint8_t* src, const uint64_t* src_off, const uint64_t* sizes, uint8_t* dst,
                       const uint64_t* dst_off, uint64_t n_obj, uint64_t dst_bytes, hipStream_t stream);

int launch_bincode_bounds(const uint64_t* blen, uint64_t n_obj, uint32_t wa, uint32_t wm, uint32_t A,
                          uint32_t flags, uint64_t* bounds, hipStream_t stream);
// decode (sizes == null): objects past the LDS scratch are listed (list,
// list_cap) and decoded by a large-object kernel from big_scratch
// (launch_bincode_big_scratch_bytes()).
int launch_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                          uint64_t n_obj, uint32_t wa, uint32_t wm, uint32_t A, uint32_t flags, uint64_t* sizes,
                          uint8_t* out, const uint64_t* ooff, uint64_t out_bytes, int* status, uint32_t* ctl, hipStream_t stream,
                          uint64_t* dbg = nullptr, uint64_t* list = nullptr, uint32_t list_cap = 0,
                          uint8_t* big_scratch = nullptr, int walk = 0);
size_t launch_bincode_big_scratch_bytes();
int launch_bincode_egest(const uint8_t* rb, uint64_t rbytes, const uint64_t* roff, uint64_t n_obj, uint32_t A,
                         uint32_t flags, uint32_t wa, uint32_t wm, uint64_t* sizes, uint8_t* out,
                         const uint64_t* ooff, uint64_t out_bytes, int* status, uint32_t* ctl, hipStream_t stream);

int launch_orswot_apply(const uint8_t* sb, uint64_t sbytes, const uint64_t* soff, uint64_t n_obj,
                        const uint64_t* obj_end, const uint32_t* kind, const uint64_t* member, const uint32_t* actor,
                        const uint64_t* counter, const uint64_t* clk_end, const uint32_t* clk_act,
                        const uint64_t* clk_ctr, uint64_t n_ops, uint64_t n_clk, uint32_t A, uint32_t flags,
                        uint8_t* out, uint64_t* ooff,
                        uint64_t out_bytes, int* status, uint32_t* ctl, uint64_t* list, uint32_t list_cap,
                        uint8_t* huge_ws, hipStream_t stream);
// HBM workspace of the apply's third tier (objects past the LDS workspaces)
size_t launch_apply_huge_scratch_bytes();

int launch_vclock_cmp(const uint64_t* a, const uint64_t* b, uint64_t n, uint32_t A, int8_t* out, hipStream_t stream);
int launch_mvreg_merge(const uint32_t* sn, const uint64_t* sclk, const uint64_t* sval, uint32_t scap,
                       const uint32_t* on, const uint64_t* oclk, const uint64_t* oval, uint32_t ocap, uint32_t* outn,
                       uint64_t* outclk, uint64_t* outval, uint32_t outcap, uint64_t n_obj, uint32_t A, int* status,
                       hipStream_t stream);

// MVReg fold (mvreg_fold.hip): reps is a host array; 1 <= n_reps <= 32, every
// cap in [1, 1024], their sum <= 2048 (api.hip checks the rest)
int launch_mvreg_fold(const crdt_mvreg_view* reps, uint32_t n_reps, uint32_t* outn, uint64_t* outclk, uint64_t* outval,
                      uint32_t outcap, uint64_t n_obj, uint32_t A, int* status, hipStream_t stream);

// MVReg op path (mvreg_apply.hip): Put lists, truncate, the read clock;
// self_cap <= out_cap within the ABI limits (api.hip)
int launch_mvreg_apply(const uint32_t* sn, const uint64_t* sclk, const uint64_t* sval, uint32_t scap,
                       const crdt_mvreg_ops& P, uint32_t* outn, uint64_t* outclk, uint64_t* outval, uint32_t outcap,
                       uint64_t n_obj, uint32_t A, int* status, hipStream_t stream);
int launch_mvreg_truncate(const uint32_t* sn, const uint64_t* sclk, const uint64_t* sval, uint32_t scap,
                          const uint64_t* clock, uint32_t* outn, uint64_t* outclk, uint64_t* outval, uint32_t outcap,
                          uint64_t n_obj, uint32_t A, int* status, hipStream_t stream);
int launch_mvreg_read_clock(const uint32_t* sn, const uint64_t* sclk, uint32_t scap, uint64_t* out, uint64_t n_obj,
                            uint32_t A, int* status, hipStream_t stream);

// LWWReg (lwwreg.hip; the ABI functions validate there too). marker_words is
// 1 or 2; merge's bitmap / count and fold's / apply's op_err may be null.
int launch_lwwreg_merge(uint64_t* sval, uint64_t* smark, const uint64_t* oval, const uint64_t* omark, uint64_t n,
                        uint32_t marker_words, uint64_t* bitmap, uint64_t* count, hipStream_t stream);
int launch_lwwreg_apply(uint64_t* sval, uint64_t* smark, const crdt_lwwreg_ops& P, uint64_t n_obj,
                        uint32_t marker_words, uint32_t* n_err, uint8_t* op_err, int* status, hipStream_t stream);
int launch_lwwreg_fold(const crdt_lwwreg_view* reps, uint32_t n_reps, uint64_t n, uint32_t marker_words,
                       uint64_t* oval, uint64_t* omark, uint32_t* n_err, hipStream_t stream);
int launch_lwwreg_from_bincode(const uint8_t* blobs, uint64_t stride, uint64_t n, uint32_t vb, uint32_t marker_words,
                               uint32_t mb0, uint32_t mb1, uint64_t* val, uint64_t* marker, hipStream_t stream);
int launch_lwwreg_to_bincode(const uint64_t* val, const uint64_t* marker, uint64_t n, uint32_t vb,
                             uint32_t marker_words, uint32_t mb0, uint32_t mb1, uint8_t* blobs, uint64_t stride,
                             int* status, hipStream_t stream);

// bincode codec of the clocks, the counters and their ops (clock_bincode.hip;
// the ABI functions validate there too). ab: actor bytes in {1, 2, 4, 8}; nc:
// clocks per object (1, or 2: PNCounter). Egest: out == nullptr is the sizes
// pass; self_n == nullptr is one clock per object.
int launch_clock_dense_from_bincode(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                    const uint64_t* blen, uint64_t n_obj, uint32_t ab, uint32_t A, uint32_t nc,
                                    uint64_t* rows, int* status, hipStream_t stream);
int launch_clock_dense_to_bincode(const uint64_t* rows, uint64_t n_obj, uint32_t A, uint32_t nc, uint32_t ab,
                                  uint64_t* sizes, uint8_t* out, const uint64_t* ooff, uint64_t out_bytes,
                                  int* status, hipStream_t stream);
int launch_clock_csr_bincode_lens(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                  const uint64_t* blen, uint64_t n_obj, uint32_t ab, uint32_t nc, uint32_t* len_p,
                                  uint32_t* len_n, int* status, hipStream_t stream);
int launch_clock_csr_from_bincode(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                  const uint64_t* blen, uint64_t n_obj, uint32_t ab, uint32_t nc,
                                  const crdt_clock_csr_out* out_p, const crdt_clock_csr_out* out_n, int* status,
                                  hipStream_t stream);
int launch_clock_csr_to_bincode(const crdt_clock_csr* self_p, const crdt_clock_csr* self_n, uint32_t ab,
                                uint64_t* sizes, uint8_t* out, const uint64_t* ooff, uint64_t out_bytes, int* status,
                                hipStream_t stream);
int launch_clock_ops_from_bincode(const uint8_t* blobs, uint64_t stride, uint64_t n_ops, uint32_t ab, bool with_dir,
                                  uint32_t* actor, uint64_t* counter, uint32_t* dir, int* status,
                                  hipStream_t stream);
int launch_clock_ops_to_bincode(const uint32_t* actor, const uint64_t* counter, const uint32_t* dir, uint64_t n_ops,
                                uint32_t ab, bool with_dir, uint8_t* blobs, uint64_t stride, int* status,
                                hipStream_t stream);

// bincode codec of the Orswot, MVReg and Map op streams (ops_bincode.hip; the
// ABI functions in api.hip validate). W: every width in {1, 2, 4, 8} (the
// caller sets the ones op_type does not use to 8); A: the arrays op_type uses
// are non-null. Egest: out == nullptr is the sizes pass.
int launch_ops_bincode_clk_lens(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                                uint64_t n_ops, uint32_t op_type, const crdt_op_widths& W, uint32_t* clk_len,
                                int* status, hipStream_t stream);
int launch_ops_from_bincode(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                            uint32_t op_type, const crdt_op_widths& W, const crdt_op_arrays& A, uint32_t* op_err,
                            int* status, hipStream_t stream);
int launch_ops_to_bincode(uint32_t op_type, const crdt_op_widths& W, const crdt_op_arrays& A, uint64_t* sizes,
                          uint8_t* out, const uint64_t* ooff, uint64_t out_bytes, int* status, hipStream_t stream);

// The read path (read.hip): exactly one of sizes / out is non-null (the sizes
// call / the write call); the same kernel, so the two cannot disagree.
int launch_orswot_read(const crdt_orswot_batch& B, const crdt_read_queries& Q, uint32_t A, uint32_t flags,
                       const crdt_read_sizes* sizes, const crdt_read_out* out, int* status, hipStream_t stream);
int launch_map_read(const crdt_map_read_view& V, const crdt_read_queries& Q, uint64_t n_obj, uint32_t A,
                    const crdt_read_sizes* sizes, const crdt_read_out* out, int* status, hipStream_t stream);
int launch_map_mvreg_get(const crdt_map_mvreg_slab& M, const crdt_read_queries& Q, uint64_t n_obj, uint32_t A,
                         uint32_t* out_n, uint64_t* out_clk, uint64_t* out_val, uint32_t out_cap, int* status,
                         hipStream_t stream);
// Map<u64, Orswot>::get's value as records: sizes non-null = the sizes call
// (present may be null), else the write call to out + ooff[j].
int launch_map_orswot_get(const crdt_map_orswot_slab& M, const crdt_read_queries& Q, uint64_t n_obj, uint32_t A,
                          uint64_t* sizes, uint32_t* present, uint8_t* out, const uint64_t* ooff, uint64_t out_bytes,
                          int* status, hipStream_t stream);
// The nested map's get value: query j's inner map as row j of out.
int launch_map_map_get(const crdt_map_map_slab& M, const crdt_read_queries& Q, uint64_t n_obj, uint32_t A,
                       const crdt_map_mvreg_slab& out, uint32_t* present, int* status, hipStream_t stream);

int launch_map_mvreg_merge(const crdt_map_mvreg_slab& S, const crdt_map_mvreg_slab& O, const crdt_map_mvreg_slab& R,
                           uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl, hipStream_t stream, int variant = 0);
// Map<u64, MVReg>::apply (map_apply.hip): R row i = S row i after its ops of P
// in order; R's capacities >= S's (api.hip)
int launch_map_mvreg_apply(const crdt_map_mvreg_slab& S, const crdt_map_mvreg_ops& P, const crdt_map_mvreg_slab& R,
                           uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl, hipStream_t stream);
// The nested map's inner pass (map_map.hip): task t merges S row tsrc[2t]
// with O row tsrc[2t + 1] (~0: an absent side) into R row t, truncated by Tb
// row t when it is non-empty (one pass: no intermediate slab).
int launch_map_mvreg_merge_tasks(const crdt_map_mvreg_slab& S, const crdt_map_mvreg_slab& O,
                                 const crdt_map_mvreg_slab& R, const uint64_t* tsrc, const uint64_t* Tb,
                                 uint64_t n_tasks, uint32_t slots, uint32_t A, int* status, uint32_t* ctl,
                                 hipStream_t stream);
size_t map_map_scratch_bytes(const crdt_map_map_slab& R, uint64_t n_obj, uint32_t A);
int launch_map_map_merge(const crdt_map_map_slab& S, const crdt_map_map_slab& O, const crdt_map_map_slab& R,
                         uint64_t n_obj, uint32_t A, uint8_t* scratch, int* status, uint32_t* ctl,
                         hipStream_t stream);
// The nested map's op path (map_map_apply.hip): R row i = S row i after its
// ops of P in order; R's capacities >= S's, scratch of
// map_map_apply_scratch_bytes(R, ..) bytes, 16-byte aligned (api.hip)
size_t map_map_apply_scratch_bytes(const crdt_map_map_slab& R, uint64_t n_obj, uint32_t A);
int launch_map_map_apply(const crdt_map_map_slab& S, const crdt_map_map_ops& P, const crdt_map_map_slab& R,
                         uint64_t n_obj, uint32_t A, uint8_t* scratch, int* status, uint32_t* ctl,
                         hipStream_t stream);
int launch_map_orswot_merge(const crdt_map_orswot_slab& S, const crdt_map_orswot_slab& O,
                            const crdt_map_orswot_slab& R, uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl,
                            hipStream_t stream, int variant = 0);
size_t map_orswot_lds_bytes(const crdt_map_orswot_slab& S, const crdt_map_orswot_slab& O, uint32_t A);
// Map<u64, Orswot>::apply (map_orswot_apply.hip): R row i = S row i after its
// ops of P in order; R's capacities >= S's and its workspace within the limit (api.hip)
int launch_map_orswot_apply(const crdt_map_orswot_slab& S, const crdt_map_orswot_ops& P,
                            const crdt_map_orswot_slab& R, uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl,
                            hipStream_t stream);
size_t map_orswot_apply_lds_bytes(const crdt_map_orswot_slab& R, uint32_t A);
constexpr size_t kMapOrswotApplyLdsMax = 65536 - 4864;  // 64 KB less the kernel's static op stage and key mirror

// Map::truncate of the three Map types (map_truncate.hip): R row i = S row i
// after Map::truncate(clk row i), clk dense [n_obj][A]; R's capacities >= S's,
// R != S (api.hip). Map<u64, Orswot>: the workspace, map_orswot_apply_lds_bytes
// of S, within kMapOrswotApplyLdsMax. The nested map: scratch of
// map_map_truncate_scratch_bytes(R, ..) bytes, 16-byte aligned.
int launch_map_mvreg_truncate(const crdt_map_mvreg_slab& S, const uint64_t* clk, const crdt_map_mvreg_slab& R,
                              uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl, hipStream_t stream);
int launch_map_orswot_truncate(const crdt_map_orswot_slab& S, const uint64_t* clk, const crdt_map_orswot_slab& R,
                               uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl, hipStream_t stream);
size_t map_map_truncate_scratch_bytes(const crdt_map_map_slab& R, uint64_t n_obj, uint32_t A);
int launch_map_map_truncate(const crdt_map_map_slab& S, const uint64_t* clk, const crdt_map_map_slab& R,
                            uint64_t n_obj, uint32_t A, uint8_t* scratch, int* status, uint32_t* ctl,
                            hipStream_t stream);

// bincode codec of MVReg / Map<u64, MVReg> over their slabs (map_bincode.hip);
// widths in {1, 2, 4, 8}, capacities within the ABI limits (api.hip). Egest:
// out == nullptr is the sizes pass.
int launch_map_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                              uint64_t n_obj, uint32_t wa, uint32_t wk, uint32_t wv, uint32_t A,
                              const crdt_map_mvreg_slab& R, int* status, hipStream_t stream);
int launch_mvreg_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                                uint64_t n_obj, uint32_t wa, uint32_t wv, uint32_t A, uint32_t* outn, uint64_t* outclk,
                                uint64_t* outval, uint32_t cap, int* status, hipStream_t stream);
int launch_map_bincode_egest(const crdt_map_mvreg_slab& S, uint64_t n_obj, uint32_t A, uint32_t wa, uint32_t wk,
                             uint32_t wv, uint64_t* sizes, uint8_t* out, const uint64_t* ooff, uint64_t out_bytes,
                             int* status, hipStream_t stream);
int launch_mvreg_bincode_egest(const uint32_t* sn, const uint64_t* sclk, const uint64_t* sval, uint32_t cap,
                               uint64_t n_obj, uint32_t A, uint32_t wa, uint32_t wv, uint64_t* sizes, uint8_t* out,
                               const uint64_t* ooff, uint64_t out_bytes, int* status, hipStream_t stream);
// The same for Map<u64, Orswot> (wm: member bytes) and the nested map (wk2:
// inner key bytes) over their slabs.
int launch_map_orswot_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                     const uint64_t* blen, uint64_t n_obj, uint32_t wa, uint32_t wk, uint32_t wm,
                                     uint32_t A, const crdt_map_orswot_slab& R, int* status, hipStream_t stream);
int launch_map_orswot_bincode_egest(const crdt_map_orswot_slab& S, uint64_t n_obj, uint32_t A, uint32_t wa,
                                    uint32_t wk, uint32_t wm, uint64_t* sizes, uint8_t* out, const uint64_t* ooff,
                                    uint64_t out_bytes, int* status, hipStream_t stream);
int launch_map_map_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                  const uint64_t* blen, uint64_t n_obj, uint32_t wa, uint32_t wk, uint32_t wk2,
                                  uint32_t wv, uint32_t A, const crdt_map_map_slab& R, int* status,
                                  hipStream_t stream);
int launch_map_map_bincode_egest(const crdt_map_map_slab& S, uint64_t n_obj, uint32_t A, uint32_t wa, uint32_t wk,
                                 uint32_t wk2, uint32_t wv, uint64_t* sizes, uint8_t* out, const uint64_t* ooff,
                                 uint64_t out_bytes, int* status, hipStream_t stream);

}  // namespace crdts_hip
