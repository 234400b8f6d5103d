// C ABI of crdts_hip (include/crdts_hip.h): argument validation, the context,
// and launches. Nothing here falls back to a CPU implementation: without a
// usable gfx950 device every device entry point returns CRDT_ENODEV/EHIP.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <vector>

#include "../../include/crdts_hip.h"
#include "ctx.h"
#include "kernels.h"
#include "map_limits.h"
#include "record_layout.h"

using namespace crdts_hip;


namespace {

inline hipStream_t S(void* s) { return (hipStream_t)s; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int set_device(crdt_ctx* ctx) {
  if (!ctx) return CRDT_EINVAL;
  return hipSetDevice(ctx->device) == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int dense(crdt_ctx* ctx, uint64_t* self, const uint64_t* other, size_t n_obj, uint64_t slots,
          void* stream) {
  if (!ctx || (n_obj && (!self || !other)) || slots == 0) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_dense_max(self, other, (uint64_t)n_obj * slots, S(stream));
}

}  // namespace

int ctx_big_scratch(crdt_ctx* ctx, size_t bytes) {
  if (ctx->big_bytes >= bytes) return CRDT_OK;
  // the previous scratch may still be read by queued kernels of this context:
  // hipFree synchronises the device first
  (void)hipFree(ctx->d_big);
  ctx->d_big = nullptr;
  ctx->big_bytes = 0;
  if (hipMalloc(&ctx->d_big, bytes) != hipSuccess) return CRDT_EHIP;
  ctx->big_bytes = bytes;
  return CRDT_OK;
}

extern "C" {

int crdt_abi_version(void) { return CRDT_ABI_VERSION; }

const char* crdt_strerror(int code) {
  switch (code) {
    case CRDT_OK: return "ok";
    case CRDT_EINVAL: return "invalid argument";
    case CRDT_ENONCANON: return "non-canonical or inconsistent record";
    case CRDT_EHIP: return "HIP runtime error";
    case CRDT_ECAPACITY: return "output capacity too small";
    case CRDT_ECOMM: return "communicator error";
    case CRDT_ENODEV: return "no usable gfx950 device";
    default: return "unknown error";
  }
}

int crdt_ctx_create(crdt_ctx** out, int device) {
  if (!out) return CRDT_EINVAL;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e == hipErrorNoDevice || (e == hipSuccess && (device < 0 || device >= n))) return CRDT_ENODEV;
  if (e != hipSuccess) return CRDT_EHIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CRDT_ENODEV;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return CRDT_ENODEV;
  if (hipSetDevice(device) != hipSuccess) return CRDT_EHIP;
  auto* c = new crdt_ctx();
  c->device = device;
  c->blocks_per_cu = 0;
  c->list_cap = kDefaultListCap;
  c->variant = 0;
  // status, ctl, the general-path list, the per-wave store sink; the deferred
  // list after it is read and written only by the two-pass join variants of
  // the diagnostic build
#ifdef CRDT_DIAG
  const size_t bytes = 64 + 8ull * kDefaultListCap + kTrashBytes + 8ull * kDeferListCap;
#else
  const size_t bytes = 64 + 8ull * kDefaultListCap + kTrashBytes;
#endif
  uint8_t* scratch = nullptr;
  if (hipMalloc(&scratch, bytes) != hipSuccess || hipMemset(scratch, 0, bytes) != hipSuccess) {
    (void)hipFree(scratch);
    delete c;
    return CRDT_EHIP;
  }
  c->d_status = (int*)scratch;
  c->d_ctl = (uint32_t*)(scratch + 16);
  c->d_list = (uint64_t*)(scratch + 64);
  *out = c;
  return CRDT_OK;
}

int crdt_ctx_destroy(crdt_ctx* ctx) {
  if (!ctx) return CRDT_EINVAL;
  (void)hipSetDevice(ctx->device);
  (void)crdt_comm_destroy(ctx);
  (void)hipFree(ctx->d_big);
  (void)hipFree(ctx->d_arena);
  (void)hipFree(ctx->d_fold);
  (void)hipFree(ctx->d_status);
  delete ctx;
  return CRDT_OK;
}

int crdt_ctx_status(crdt_ctx* ctx, void* stream) {
  int rc = set_device(ctx);
  if (rc) return rc;
  if (hipStreamSynchronize(S(stream)) != hipSuccess) return CRDT_EHIP;
  int st = 0;
  if (hipMemcpy(&st, ctx->d_status, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return CRDT_EHIP;
  if (st != 0 && hipMemset(ctx->d_status, 0, sizeof(int)) != hipSuccess) return CRDT_EHIP;
  return st;
}

int crdt_ctx_set_arena_limit(crdt_ctx* ctx, size_t max_bytes) {
  if (!ctx) return CRDT_EINVAL;
  ctx->arena_limit = max_bytes;
  return CRDT_OK;
}

int crdt_ctx_set_list_cap(crdt_ctx* ctx, uint32_t cap) {
  if (!ctx || cap > kDefaultListCap) return CRDT_EINVAL;
  ctx->list_cap = cap;
  return CRDT_OK;
}

#ifdef CRDT_DIAG
// Diagnostic build only (-DCRDT_DIAG, lib/libcrdts_hip_diag.so, used by
// tools/): copy the context's list buffer
// (holds per-wave phase stamps after a variant-109 launch).
int crdt_ctx_debug_read(crdt_ctx* ctx, uint64_t* h_out, size_t n, void* stream) {
  if (!ctx || !h_out || n > 8ull * kDefaultListCap / 8) return CRDT_EINVAL;
  if (hipMemcpyAsync(h_out, ctx->d_list, 8 * n, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return CRDT_EHIP;
  return CRDT_OK;
}

// Orswot kernel variant (diagnostic build only).
int crdt_ctx_set_variant(crdt_ctx* ctx, int v) {
  if (!ctx || v < 0) return CRDT_EINVAL;
  ctx->variant = v;
  return CRDT_OK;
}

// Workgroups per CU for the Orswot kernel (diagnostic build only).
int crdt_ctx_set_blocks_per_cu(crdt_ctx* ctx, int k) {
  if (!ctx || k < 0 || k > 64) return CRDT_EINVAL;  // 0 = the variant's occupancy
  ctx->blocks_per_cu = k;
  return CRDT_OK;
}
#endif  // CRDT_DIAG

int crdt_vclock_dense_merge(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                            uint32_t n_actors, void* stream) {
  return dense(ctx, d_self, d_other, n_obj, n_actors, stream);
}
int crdt_gcounter_merge(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                        uint32_t n_actors, void* stream) {
  return dense(ctx, d_self, d_other, n_obj, n_actors, stream);
}
int crdt_pncounter_merge(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                         uint32_t n_actors, void* stream) {
  return dense(ctx, d_self, d_other, n_obj, 2ull * n_actors, stream);
}

namespace {
int csr_args_ok(const crdt_clock_csr* s, const crdt_clock_csr* o, const crdt_clock_csr_out* out) {
  if (!s || !o || !out || s->n_obj != o->n_obj) return CRDT_EINVAL;
  if (s->n_obj && (!s->off || !s->len || !o->off || !o->len || !out->off || !out->len)) return CRDT_EINVAL;
  if (s->n_entries && (!s->act || !s->ctr)) return CRDT_EINVAL;
  if (o->n_entries && (!o->act || !o->ctr)) return CRDT_EINVAL;
  if (out->n_entries && (!out->act || !out->ctr)) return CRDT_EINVAL;
  if (out->n_entries < s->n_entries + o->n_entries) return CRDT_ECAPACITY;
  return CRDT_OK;
}
}  // namespace

int crdt_vclock_csr_merge(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                          const crdt_clock_csr_out* out, void* stream) {
  if (!ctx) return CRDT_EINVAL;
  int rc = csr_args_ok(self, other, out);
  if (rc || (rc = set_device(ctx))) return rc;
  return launch_clock_csr_merge(&self, &other, &out, 1, ctx->d_status, S(stream));
}
int crdt_gcounter_csr_merge(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                            const crdt_clock_csr_out* out, void* stream) {
  return crdt_vclock_csr_merge(ctx, self, other, out, stream);
}
int crdt_pncounter_csr_merge(crdt_ctx* ctx, const crdt_clock_csr* self_p, const crdt_clock_csr* self_n,
                             const crdt_clock_csr* other_p, const crdt_clock_csr* other_n,
                             const crdt_clock_csr_out* out_p, const crdt_clock_csr_out* out_n, void* stream) {
  if (!ctx || !self_p || !self_n || self_p->n_obj != self_n->n_obj) return CRDT_EINVAL;
  int rc = csr_args_ok(self_p, other_p, out_p);
  if (rc || (rc = csr_args_ok(self_n, other_n, out_n)) || (rc = set_device(ctx))) return rc;
  const crdt_clock_csr* s[2] = {self_p, self_n};
  const crdt_clock_csr* o[2] = {other_p, other_n};
  const crdt_clock_csr_out* w[2] = {out_p, out_n};
  return launch_clock_csr_merge(s, o, w, 2, ctx->d_status, S(stream));
}

// ---- the clocks' op path (clock_ops.hip)
namespace {
// the op batch of an apply (need_counter; need_dir: PNCounter) or of a get
bool clock_ops_ok(const crdt_clock_ops* p, size_t n_obj, bool need_counter, bool need_dir) {
  if (!p || (n_obj && !p->obj_end)) return false;
  if (p->n_ops && (!p->actor || (need_counter && !p->counter) || (need_dir && !p->dir))) return false;
  return true;
}
bool clock_ops_alias(const crdt_clock_ops* p, const void* w) {
  return w && (w == p->obj_end || w == p->actor || w == p->counter || w == p->dir);
}
int dense_apply(crdt_ctx* ctx, uint64_t* self, const crdt_clock_ops* ops, size_t n_obj, uint32_t n_actors, bool pn,
                void* stream) {
  if (!ctx || n_actors == 0 || !clock_ops_ok(ops, n_obj, true, pn) || (n_obj && !self)) return CRDT_EINVAL;
  if (n_obj && clock_ops_alias(ops, self)) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_dense_clock_apply(self, *ops, pn, n_obj, n_actors, ctx->d_status, S(stream));
}
int dense_binop(crdt_ctx* ctx, int op, uint64_t* self, const uint64_t* other, size_t n_obj, uint32_t n_actors,
                void* stream) {
  if (!ctx || n_actors == 0 || (n_obj && (!self || !other || self == other))) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_dense_clock_binop(op, self, other, (uint64_t)n_obj * n_actors, S(stream));
}
int dense_value(crdt_ctx* ctx, const uint64_t* rows, uint64_t* out, size_t n_obj, uint32_t n_actors, bool pn,
                void* stream) {
  if (!ctx || n_actors == 0 || (n_obj && (!rows || !out || (const uint64_t*)out == rows))) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_dense_clock_value(rows, out, pn, n_obj, n_actors, S(stream));
}
bool csr_in_ok(const crdt_clock_csr* s) {
  return s && !(s->n_obj && (!s->off || !s->len)) && !(s->n_entries && (!s->act || !s->ctr));
}
bool csr_out_ok(const crdt_clock_csr_out* w, size_t n_obj) {
  return w && !(n_obj && (!w->off || !w->len)) && !(w->n_entries && (!w->act || !w->ctr));
}
bool csr_alias(const crdt_clock_csr* s, const crdt_clock_csr_out* w) {
  const void* in[4] = {s->off, s->len, s->act, s->ctr};
  const void* out[4] = {w->off, w->len, w->act, w->ctr};
  for (const void* a : in)
    for (const void* b : out)
      if (a && a == b) return true;
  return false;
}
int csr_filter(crdt_ctx* ctx, int op, const crdt_clock_csr* self, const crdt_clock_csr* other,
               const crdt_clock_csr_out* out, void* stream) {
  if (!ctx || !csr_in_ok(self) || !csr_in_ok(other) || self->n_obj != other->n_obj || !csr_out_ok(out, self->n_obj))
    return CRDT_EINVAL;
  if (self->n_obj && (csr_alias(self, out) || csr_alias(other, out))) return CRDT_EINVAL;
  if (out->n_entries < self->n_entries) return CRDT_ECAPACITY;
  if (self->n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_csr_filter(op, *self, *other, *out, ctx->d_status, S(stream));
}
}  // namespace

int crdt_vclock_dense_apply(crdt_ctx* ctx, uint64_t* d_self, const crdt_clock_ops* ops, size_t n_obj,
                            uint32_t n_actors, void* stream) {
  return dense_apply(ctx, d_self, ops, n_obj, n_actors, false, stream);
}
int crdt_gcounter_apply(crdt_ctx* ctx, uint64_t* d_self, const crdt_clock_ops* ops, size_t n_obj, uint32_t n_actors,
                        void* stream) {
  return dense_apply(ctx, d_self, ops, n_obj, n_actors, false, stream);
}
int crdt_pncounter_apply(crdt_ctx* ctx, uint64_t* d_self, const crdt_clock_ops* ops, size_t n_obj, uint32_t n_actors,
                         void* stream) {
  return dense_apply(ctx, d_self, ops, n_obj, n_actors, true, stream);
}
int crdt_vclock_dense_truncate(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                               uint32_t n_actors, void* stream) {
  return dense_binop(ctx, kClockTruncate, d_self, d_other, n_obj, n_actors, stream);
}
int crdt_vclock_dense_subtract(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                               uint32_t n_actors, void* stream) {
  return dense_binop(ctx, kClockSubtract, d_self, d_other, n_obj, n_actors, stream);
}
int crdt_vclock_dense_intersection(crdt_ctx* ctx, uint64_t* d_self, const uint64_t* d_other, size_t n_obj,
                                   uint32_t n_actors, void* stream) {
  return dense_binop(ctx, kClockIntersection, d_self, d_other, n_obj, n_actors, stream);
}
int crdt_gcounter_value(crdt_ctx* ctx, const uint64_t* d_rows, uint64_t* d_out, size_t n_obj, uint32_t n_actors,
                        void* stream) {
  return dense_value(ctx, d_rows, d_out, n_obj, n_actors, false, stream);
}
int crdt_pncounter_value(crdt_ctx* ctx, const uint64_t* d_rows, int64_t* d_out, size_t n_obj, uint32_t n_actors,
                         void* stream) {
  return dense_value(ctx, d_rows, (uint64_t*)d_out, n_obj, n_actors, true, stream);
}
int crdt_vclock_dense_get(crdt_ctx* ctx, const uint64_t* d_rows, const crdt_clock_ops* queries, uint64_t* d_out,
                          size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || n_actors == 0 || !clock_ops_ok(queries, n_obj, false, false)) return CRDT_EINVAL;
  if (n_obj && (!d_rows || (queries->n_ops && !d_out))) return CRDT_EINVAL;
  if (n_obj && d_out && ((const uint64_t*)d_out == d_rows || clock_ops_alias(queries, d_out))) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_dense_clock_get(d_rows, *queries, d_out, n_obj, n_actors, ctx->d_status, S(stream));
}
int crdt_vclock_csr_truncate(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                             const crdt_clock_csr_out* out, void* stream) {
  return csr_filter(ctx, kClockTruncate, self, other, out, stream);
}
int crdt_vclock_csr_subtract(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                             const crdt_clock_csr_out* out, void* stream) {
  return csr_filter(ctx, kClockSubtract, self, other, out, stream);
}
int crdt_vclock_csr_intersection(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_csr* other,
                                 const crdt_clock_csr_out* out, void* stream) {
  return csr_filter(ctx, kClockIntersection, self, other, out, stream);
}
int crdt_vclock_csr_apply(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_ops* ops,
                          const crdt_clock_csr_out* out, void* stream) {
  if (!ctx || !csr_in_ok(self) || !clock_ops_ok(ops, self->n_obj, true, false) || !csr_out_ok(out, self->n_obj))
    return CRDT_EINVAL;
  if (self->n_obj) {
    if (csr_alias(self, out)) return CRDT_EINVAL;
    for (const void* w : {(const void*)out->off, (const void*)out->len, (const void*)out->act, (const void*)out->ctr})
      if (clock_ops_alias(ops, w)) return CRDT_EINVAL;
  }
  if (out->n_entries < self->n_entries + ops->n_ops) return CRDT_ECAPACITY;
  if (self->n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  // the long paths' scratch (more than 64 dots or entries in one object)
  if (ops->n_ops && (rc = ctx_big_scratch(ctx, clock_csr_apply_scratch_bytes(*ops)))) return rc;
  return launch_clock_csr_apply(*self, *ops, *out, ops->n_ops ? ctx->d_big : nullptr, ctx->d_status, S(stream));
}
int crdt_gcounter_csr_apply(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_ops* ops,
                            const crdt_clock_csr_out* out, void* stream) {
  return crdt_vclock_csr_apply(ctx, self, ops, out, stream);
}
int crdt_gcounter_csr_value(crdt_ctx* ctx, const crdt_clock_csr* self, uint64_t* d_out, void* stream) {
  if (!ctx || !csr_in_ok(self) || (self->n_obj && (!d_out || (const uint64_t*)d_out == self->ctr ||
                                                   (const uint64_t*)d_out == self->off)))
    return CRDT_EINVAL;
  if (self->n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_csr_value(*self, d_out, ctx->d_status, S(stream));
}
int crdt_vclock_csr_get(crdt_ctx* ctx, const crdt_clock_csr* self, const crdt_clock_ops* queries, uint64_t* d_out,
                        void* stream) {
  if (!ctx || !csr_in_ok(self) || !clock_ops_ok(queries, self->n_obj, false, false)) return CRDT_EINVAL;
  if (self->n_obj && queries->n_ops &&
      (!d_out || (const uint64_t*)d_out == self->ctr || (const uint64_t*)d_out == self->off ||
       clock_ops_alias(queries, d_out)))
    return CRDT_EINVAL;
  if (self->n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_csr_get(*self, *queries, d_out, ctx->d_status, S(stream));
}

// ---- the clocks' fold (clock_fold.hip)
int crdt_clock_dense_fold(crdt_ctx* ctx, const uint64_t* const* h_rows, uint32_t n_reps, uint64_t* d_out, size_t n_obj,
                          uint32_t n_slots, void* stream) {
  if (!ctx || !h_rows || n_reps == 0 || n_reps > CRDT_CLOCK_FOLD_MAX_REPS || n_slots == 0) return CRDT_EINVAL;
  if (n_obj) {
    if (!d_out) return CRDT_EINVAL;
    for (uint32_t r = 0; r < n_reps; ++r)
      if (!h_rows[r]) return CRDT_EINVAL;
  }
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_dense_fold(h_rows, n_reps, d_out, (uint64_t)n_obj * n_slots, S(stream));
}
int crdt_clock_csr_fold(crdt_ctx* ctx, const crdt_clock_csr* h_reps, uint32_t n_reps, const crdt_clock_csr_out* out,
                        void* stream) {
  if (!ctx || !h_reps || n_reps == 0 || n_reps > CRDT_CLOCK_FOLD_MAX_REPS) return CRDT_EINVAL;
  const size_t n_obj = h_reps[0].n_obj;
  size_t total = 0;
  for (uint32_t r = 0; r < n_reps; ++r) {
    if (!csr_in_ok(&h_reps[r]) || h_reps[r].n_obj != n_obj) return CRDT_EINVAL;
    total += h_reps[r].n_entries;
  }
  if (!csr_out_ok(out, n_obj)) return CRDT_EINVAL;
  for (uint32_t r = 0; n_obj && r < n_reps; ++r)
    if (csr_alias(&h_reps[r], out)) return CRDT_EINVAL;
  if (out->n_entries < total) return CRDT_ECAPACITY;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_csr_fold(h_reps, n_reps, *out, ctx->d_status, S(stream));
}

int crdt_orswot_truncate(crdt_ctx* ctx, const crdt_orswot_batch* self, const crdt_clock_csr* clocks,
                         uint32_t n_actors, uint32_t flags, uint8_t* d_out, uint64_t* d_out_off, size_t out_bytes,
                         void* stream) {
  if (!ctx || !self || !clocks || n_actors == 0 || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK) ||
      clocks->n_obj != self->n_obj)
    return CRDT_EINVAL;
  if (self->n_obj == 0) return CRDT_OK;
  if (!self->base || !self->off || !clocks->off || !clocks->len || !d_out || !d_out_off || !aligned16(d_out))
    return CRDT_EINVAL;
  if (clocks->n_entries && (!clocks->act || !clocks->ctr)) return CRDT_EINVAL;
  if (out_bytes < self->bytes) return CRDT_ECAPACITY;
  // out must not alias the input: the HBM form compacts sections toward lower
  // offsets while other lanes still read them
  const uintptr_t ib = (uintptr_t)self->base, ob = (uintptr_t)d_out;
  if (ob < ib + self->bytes && ib < ob + out_bytes) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_orswot_truncate(*self, *clocks, n_actors, flags, d_out, d_out_off, out_bytes, ctx->d_status,
                                ctx->d_ctl, ctx->d_list, ctx->list_cap, S(stream));
}

int crdt_dense_merge_host(crdt_ctx* ctx, uint64_t* h_self, const uint64_t* h_other, size_t n_obj, uint32_t n_slots) {
  if (!ctx || n_slots == 0 || (n_obj && (!h_self || !h_other))) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  const size_t bytes = 8ull * n_obj * n_slots;
  uint64_t *dS = nullptr, *dO = nullptr;
  hipStream_t st = nullptr;
  bool ok = hipStreamCreate(&st) == hipSuccess && hipMalloc(&dS, bytes) == hipSuccess &&
            hipMalloc(&dO, bytes) == hipSuccess &&
            hipMemcpyAsync(dS, h_self, bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(dO, h_other, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok) rc = launch_dense_max(dS, dO, (uint64_t)n_obj * n_slots, st);
  ok = ok && rc == CRDT_OK && hipMemcpyAsync(h_self, dS, bytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipStreamSynchronize(st) == hipSuccess;
  (void)hipFree(dS);
  (void)hipFree(dO);
  if (st) (void)hipStreamDestroy(st);
  return ok ? CRDT_OK : (rc ? rc : CRDT_EHIP);
}

int crdt_orswot_merge(crdt_ctx* ctx, const crdt_orswot_batch* self, const crdt_orswot_batch* other,
                      uint8_t* d_out_base, uint64_t* d_out_off, size_t out_bytes, uint32_t n_actors,
                      void* stream) {
  return crdt_orswot_merge_ex(ctx, self, other, d_out_base, d_out_off, out_bytes, n_actors, 0u, stream);
}

int crdt_orswot_merge_ex(crdt_ctx* ctx, const crdt_orswot_batch* self, const crdt_orswot_batch* other,
                         uint8_t* d_out_base, uint64_t* d_out_off, size_t out_bytes, uint32_t n_actors,
                         uint32_t flags, void* stream) {
  if (!ctx || !self || !other || n_actors == 0 || self->n_obj != other->n_obj) return CRDT_EINVAL;
  if (flags & ~CRDT_ORSWOT_SPARSE_CLOCK) return CRDT_EINVAL;
  if (self->n_obj == 0) return CRDT_OK;
  if (!self->base || !self->off || !other->base || !other->off || !d_out_base || !d_out_off)
    return CRDT_EINVAL;
  if (!aligned16(self->base) || !aligned16(other->base) || !aligned16(d_out_base)) return CRDT_EINVAL;
  if (out_bytes < self->bytes + other->bytes) return CRDT_ECAPACITY;
  int rc = set_device(ctx);
  if (rc) return rc;
  if (flags & CRDT_ORSWOT_SPARSE_CLOCK)
    return launch_orswot_merge_sparse(self->base, self->off, self->bytes, other->base, other->off, other->bytes,
                                      d_out_base, d_out_off, out_bytes, self->n_obj, n_actors, ctx->d_status,
                                      ctx->d_ctl, ctx->d_list, ctx->list_cap, S(stream),
                                      ctx->variant >= 201 && ctx->variant <= 211 ? ctx->variant - 200 : 0,
                                      &ctx->join_seq);
  return launch_orswot_merge(self->base, self->off, self->bytes, other->base, other->off,
                             other->bytes, d_out_base, d_out_off, out_bytes, self->n_obj, n_actors,
                             ctx->d_status, ctx->d_ctl, ctx->d_list, ctx->list_cap, S(stream),
                             ctx->blocks_per_cu, ctx->variant, &ctx->join_seq);
}

int crdt_orswot_fold(crdt_ctx* ctx, const crdt_orswot_batch* reps, uint32_t n_reps, uint32_t n_actors,
                     uint32_t flags, uint8_t* d_out, uint64_t* d_out_off, size_t out_bytes, void* stream) {
  if (!ctx || !reps || n_reps == 0 || n_actors == 0 || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK)) return CRDT_EINVAL;
  const size_t n = reps[0].n_obj;
  size_t total = 0;
  for (uint32_t r = 0; r < n_reps; ++r) {
    if (reps[r].n_obj != n) return CRDT_EINVAL;
    if (n && (!reps[r].base || !reps[r].off || !aligned16(reps[r].base))) return CRDT_EINVAL;
    total += reps[r].bytes;
  }
  if (n == 0) return CRDT_OK;
  if (!d_out || !d_out_off || !aligned16(d_out)) return CRDT_EINVAL;
  if (out_bytes < total) return CRDT_ECAPACITY;
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = S(stream);
  if (n_reps == 1) {  // the batch itself, at its own offsets
    if (hipMemcpyAsync(d_out, reps[0].base, reps[0].bytes, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_out_off, reps[0].off, 8 * n, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return CRDT_EHIP;
    return launch_orswot_validate(d_out, d_out_off, out_bytes, n, n_actors, flags, ctx->d_status, st);
  }
  // intermediate batches: two of the first n_reps - 1 batches' bytes together
  // (an accumulator never outgrows its inputs) plus their offsets
  const size_t acc_cap = (total - reps[n_reps - 1].bytes + 255) & ~size_t(255);
  const size_t need = 2 * acc_cap + 2 * ((8 * n + 255) & ~size_t(255));
  if (n_reps > 2 && ctx->fold_bytes < need) {
    (void)hipFree(ctx->d_fold);
    ctx->d_fold = nullptr;
    ctx->fold_bytes = 0;
    if (hipMalloc(&ctx->d_fold, need) != hipSuccess) return CRDT_EHIP;
    ctx->fold_bytes = need;
  }
  uint8_t* buf[2] = {ctx->d_fold, ctx->d_fold + acc_cap};
  uint64_t* boff[2] = {(uint64_t*)(ctx->d_fold + 2 * acc_cap),
                       (uint64_t*)(ctx->d_fold + 2 * acc_cap + ((8 * n + 255) & ~size_t(255)))};
  const uint8_t* acc = reps[0].base;
  const uint64_t* acc_off = reps[0].off;
  uint64_t acc_bytes = reps[0].bytes;
  for (uint32_t r = 1; r < n_reps && !rc; ++r) {  // ((r0 ⊔ r1) ⊔ r2) ⊔ ..., each step one batched merge
    const bool last = r + 1 == n_reps;
    uint8_t* o = last ? d_out : buf[r & 1u];
    uint64_t* oo = last ? d_out_off : boff[r & 1u];
    const uint64_t cap = last ? out_bytes : acc_bytes + reps[r].bytes;
    rc = (flags & CRDT_ORSWOT_SPARSE_CLOCK)
             ? launch_orswot_merge_sparse(acc, acc_off, acc_bytes, reps[r].base, reps[r].off, reps[r].bytes, o, oo,
                                          cap, n, n_actors, ctx->d_status, ctx->d_ctl, ctx->d_list, ctx->list_cap,
                                          st, 0, &ctx->join_seq)
             : launch_orswot_merge(acc, acc_off, acc_bytes, reps[r].base, reps[r].off, reps[r].bytes, o, oo, cap, n,
                                   n_actors, ctx->d_status, ctx->d_ctl, ctx->d_list, ctx->list_cap, st, 0, 0,
                                   &ctx->join_seq);
    acc = o;
    acc_off = oo;
    acc_bytes = cap;
  }
  return rc;
}

int crdt_orswot_validate(crdt_ctx* ctx, const crdt_orswot_batch* batch, uint32_t n_actors,
                         void* stream) {
  return crdt_orswot_validate_ex(ctx, batch, n_actors, 0u, stream);
}

int crdt_orswot_validate_ex(crdt_ctx* ctx, const crdt_orswot_batch* batch, uint32_t n_actors, uint32_t flags,
                            void* stream) {
  if (!ctx || !batch || n_actors == 0 || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK)) return CRDT_EINVAL;
  if (batch->n_obj && (!batch->base || !batch->off)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_orswot_validate(batch->base, batch->off, batch->bytes, batch->n_obj, n_actors, flags,
                                ctx->d_status, S(stream));
}

size_t crdt_orswot_compact_scratch_bytes(size_t n_obj) {
  size_t temp = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, temp, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                   (int)(n_obj ? n_obj : 1));
  return ((8 * n_obj + 255) & ~size_t(255)) + temp + 256;
}

uint64_t crdt_ctx_host_syncs(const crdt_ctx* ctx) { return ctx ? ctx->host_syncs : 0ull; }

int crdt_orswot_compact(crdt_ctx* ctx, const crdt_orswot_batch* src, uint8_t* d_dst,
                        uint64_t* d_dst_off, size_t dst_bytes, void* d_scratch, void* stream) {
  if (!ctx || !src || (src->n_obj && (!src->base || !src->off || !d_dst || !d_dst_off || !d_scratch)))
    return CRDT_EINVAL;
  if (src->n_obj == 0) return CRDT_OK;
  if (src->n_obj > 0x7FFFFFFFull) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  uint64_t* sizes = (uint64_t*)d_scratch;
  uint8_t* temp = (uint8_t*)d_scratch + ((8 * src->n_obj + 255) & ~size_t(255));
  size_t temp_bytes = crdt_orswot_compact_scratch_bytes(src->n_obj) -
                      ((8 * src->n_obj + 255) & ~size_t(255)) - 256;
  if ((rc = launch_record_sizes(src->base, src->off, src->bytes, src->n_obj, sizes, ctx->d_status, S(stream))))
    return rc;
  if (hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, sizes, d_dst_off, (int)src->n_obj,
                                       S(stream)) != hipSuccess)
    return CRDT_EHIP;
  // bound check: last offset + last size <= dst_bytes (host round trip is fine here)
  uint64_t last_off = 0, last_size = 0;
  if (hipMemcpyAsync(&last_off, d_dst_off + src->n_obj - 1, 8, hipMemcpyDeviceToHost, S(stream)) !=
          hipSuccess ||
      hipMemcpyAsync(&last_size, sizes + src->n_obj - 1, 8, hipMemcpyDeviceToHost, S(stream)) !=
          hipSuccess ||
      hipStreamSynchronize(S(stream)) != hipSuccess)
    return CRDT_EHIP;
  if (last_off + last_size > dst_bytes) return CRDT_ECAPACITY;
  return launch_record_copy(src->base, src->off, sizes, d_dst, d_dst_off, src->n_obj, dst_bytes, S(stream));
}

int crdt_orswot_merge_host(crdt_ctx* ctx, const uint8_t* h_self_base, const uint64_t* h_self_off,
                           size_t self_bytes, const uint8_t* h_other_base,
                           const uint64_t* h_other_off, size_t other_bytes, size_t n_obj,
                           uint32_t n_actors, uint8_t* h_out_base, uint64_t* h_out_off,
                           size_t h_out_bytes, size_t* h_out_used) {
  if (!ctx || n_actors == 0) return CRDT_EINVAL;
  if (n_obj == 0) {
    if (h_out_used) *h_out_used = 0;
    return CRDT_OK;
  }
  if (!h_self_base || !h_self_off || !h_other_base || !h_other_off || !h_out_base || !h_out_off)
    return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  size_t sb = (self_bytes + 15) & ~size_t(15), ob = (other_bytes + 15) & ~size_t(15);
  size_t outb = sb + ob;
  uint8_t *dL = nullptr, *dR = nullptr, *dO = nullptr;
  uint64_t *dLo = nullptr, *dRo = nullptr, *dOo = nullptr;
  hipStream_t st = nullptr;
  auto cleanup = [&]() {
    (void)hipFree(dL); (void)hipFree(dR); (void)hipFree(dO);
    (void)hipFree(dLo); (void)hipFree(dRo); (void)hipFree(dOo);
    if (st) (void)hipStreamDestroy(st);
  };
  if (hipStreamCreate(&st) != hipSuccess || hipMalloc(&dL, sb) != hipSuccess ||
      hipMalloc(&dR, ob) != hipSuccess || hipMalloc(&dO, outb) != hipSuccess ||
      hipMalloc(&dLo, 8 * n_obj) != hipSuccess || hipMalloc(&dRo, 8 * n_obj) != hipSuccess ||
      hipMalloc(&dOo, 8 * n_obj) != hipSuccess) {
    cleanup();
    return CRDT_EHIP;
  }
  bool ok = hipMemcpyAsync(dL, h_self_base, self_bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(dR, h_other_base, other_bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(dLo, h_self_off, 8 * n_obj, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(dRo, h_other_off, 8 * n_obj, hipMemcpyHostToDevice, st) == hipSuccess;
  if (!ok) { cleanup(); return CRDT_EHIP; }
  crdt_orswot_batch Lb = {dL, dLo, n_obj, sb}, Rb = {dR, dRo, n_obj, ob};
  rc = crdt_orswot_merge(ctx, &Lb, &Rb, dO, dOo, outb, n_actors, st);
  if (rc == CRDT_OK) rc = crdt_ctx_status(ctx, st);
  if (rc != CRDT_OK) { cleanup(); return rc; }
  std::vector<uint64_t> offs(n_obj);
  std::vector<uint8_t> out(outb);
  ok = hipMemcpyAsync(offs.data(), dOo, 8 * n_obj, hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipMemcpyAsync(out.data(), dO, outb, hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipStreamSynchronize(st) == hipSuccess;
  cleanup();
  if (!ok) return CRDT_EHIP;
  size_t pos = 0;
  for (size_t i = 0; i < n_obj; ++i) {
    uint32_t size;
    std::memcpy(&size, out.data() + offs[i], 4);
    if (pos + size > h_out_bytes) return CRDT_ECAPACITY;
    std::memcpy(h_out_base + pos, out.data() + offs[i], size);
    h_out_off[i] = pos;
    pos += size;
  }
  if (h_out_used) *h_out_used = pos;
  return CRDT_OK;
}

// ---------------------------------------------------------------- bincode codec
namespace {
bool bc_width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }
}  // namespace

int crdt_orswot_bincode_record_sizes(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes,
                                     const uint64_t* d_blob_off, const uint64_t* d_blob_len, size_t n_obj,
                                     uint32_t actor_bytes, uint32_t member_bytes, uint32_t n_actors,
                                     uint32_t flags, uint64_t* d_sizes, void* stream) {
  if (!ctx || (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !d_sizes)) || n_actors == 0 ||
      !bc_width_ok(actor_bytes) || !bc_width_ok(member_bytes) || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK))
    return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_bincode_ingest(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, member_bytes,
                               n_actors, flags, d_sizes, nullptr, nullptr, 0, ctx->d_status, ctx->d_ctl, S(stream));
}

int crdt_orswot_bincode_record_bounds(crdt_ctx* ctx, const uint64_t* d_blob_len, size_t n_obj,
                                      uint32_t actor_bytes, uint32_t member_bytes, uint32_t n_actors, uint32_t flags,
                                      uint64_t* d_bounds, void* stream) {
  if (!ctx || (n_obj && (!d_blob_len || !d_bounds)) || !bc_width_ok(actor_bytes) || !bc_width_ok(member_bytes) ||
      n_actors == 0 || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK))
    return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_bincode_bounds(d_blob_len, n_obj, actor_bytes, member_bytes, n_actors, flags, d_bounds, S(stream));
}

int crdt_orswot_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes,
                             const uint64_t* d_blob_off, const uint64_t* d_blob_len, size_t n_obj,
                             uint32_t actor_bytes, uint32_t member_bytes, uint32_t n_actors, uint32_t flags,
                             uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes, void* stream) {
  if (!ctx || (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !d_out || !d_out_off)) || n_actors == 0 ||
      !bc_width_ok(actor_bytes) || !bc_width_ok(member_bytes) || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK) ||
      !aligned16(d_out))
    return CRDT_EINVAL;
  int rc = set_device(ctx);
  const size_t big = launch_apply_huge_scratch_bytes() > launch_bincode_big_scratch_bytes()
                         ? launch_apply_huge_scratch_bytes() : launch_bincode_big_scratch_bytes();
  if (rc || (rc = ctx_big_scratch(ctx, big))) return rc;
  return launch_bincode_ingest(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, member_bytes,
                               n_actors, flags, nullptr, d_out, d_out_off, out_bytes, ctx->d_status, ctx->d_ctl, S(stream),
                               ctx->variant == 301 ? ctx->d_list : nullptr, ctx->d_list, ctx->list_cap, ctx->d_big,
                               ctx->variant == 305 ? 1 : ctx->variant == 304 ? 2 : ctx->variant == 306 ? 3 : 0);
}

int crdt_orswot_bincode_sizes(crdt_ctx* ctx, const crdt_orswot_batch* batch, uint32_t n_actors, uint32_t flags,
                              uint32_t actor_bytes, uint32_t member_bytes, uint64_t* d_sizes, void* stream) {
  if (!ctx || !batch || (batch->n_obj && (!batch->base || !batch->off || !d_sizes)) || n_actors == 0 ||
      !bc_width_ok(actor_bytes) || !bc_width_ok(member_bytes) || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK) ||
      (batch->n_obj && !aligned16(batch->base)))
    return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_bincode_egest(batch->base, batch->bytes, batch->off, batch->n_obj, n_actors, flags, actor_bytes,
                              member_bytes, d_sizes, nullptr, nullptr, 0, ctx->d_status, ctx->d_ctl, S(stream));
}

int crdt_orswot_to_bincode(crdt_ctx* ctx, const crdt_orswot_batch* batch, uint32_t n_actors, uint32_t flags,
                           uint32_t actor_bytes, uint32_t member_bytes, uint8_t* d_out,
                           const uint64_t* d_out_off, size_t out_bytes, void* stream) {
  if (!ctx || !batch || (batch->n_obj && (!batch->base || !batch->off || !d_out || !d_out_off)) ||
      n_actors == 0 || !bc_width_ok(actor_bytes) || !bc_width_ok(member_bytes) ||
      (flags & ~CRDT_ORSWOT_SPARSE_CLOCK) || (batch->n_obj && (!aligned16(batch->base) || !aligned16(d_out))))
    return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_bincode_egest(batch->base, batch->bytes, batch->off, batch->n_obj, n_actors, flags, actor_bytes,
                              member_bytes, nullptr, d_out, d_out_off, out_bytes, ctx->d_status, ctx->d_ctl, S(stream));
}

int crdt_orswot_apply(crdt_ctx* ctx, const crdt_orswot_batch* self, const crdt_orswot_ops* ops, uint32_t n_actors,
                      uint32_t flags, uint8_t* d_out, uint64_t* d_out_off, size_t out_bytes, void* stream) {
  if (!ctx || !self || !ops || n_actors == 0 || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK)) return CRDT_EINVAL;
  if (self->n_obj && (!self->base || !self->off || !ops->obj_end || !d_out || !d_out_off || !aligned16(d_out)))
    return CRDT_EINVAL;
  if (ops->n_ops && (!ops->kind || !ops->member || !ops->actor || !ops->counter || !ops->clk_end))
    return CRDT_EINVAL;
  if (ops->n_clk && (!ops->clk_act || !ops->clk_ctr)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  const size_t big = launch_apply_huge_scratch_bytes() > launch_bincode_big_scratch_bytes()
                         ? launch_apply_huge_scratch_bytes() : launch_bincode_big_scratch_bytes();
  if ((rc = ctx_big_scratch(ctx, big))) return rc;
  return launch_orswot_apply(self->base, self->bytes, self->off, self->n_obj, ops->obj_end, ops->kind, ops->member,
                             ops->actor, ops->counter, ops->clk_end, ops->clk_act, ops->clk_ctr, ops->n_ops, ops->n_clk,
                             n_actors, flags,
                             d_out, d_out_off, out_bytes, ctx->d_status, ctx->d_ctl, ctx->d_list, ctx->list_cap,
                             ctx->d_big, S(stream));
}

int crdt_vclock_partial_cmp(crdt_ctx* ctx, const uint64_t* d_a, const uint64_t* d_b, size_t n, uint32_t n_actors,
                            int8_t* d_out, void* stream) {
  if (!ctx || n_actors == 0 || (n && (!d_a || !d_b || !d_out))) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_vclock_cmp(d_a, d_b, n, n_actors, d_out, S(stream));
}

int crdt_mvreg_merge(crdt_ctx* ctx, const uint32_t* d_self_n, const uint64_t* d_self_clk, const uint64_t* d_self_val,
                     uint32_t self_cap, const uint32_t* d_other_n, const uint64_t* d_other_clk,
                     const uint64_t* d_other_val, uint32_t other_cap, uint32_t* d_out_n, uint64_t* d_out_clk,
                     uint64_t* d_out_val, uint32_t out_cap, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || n_actors == 0 || self_cap == 0 || other_cap == 0 || self_cap > 1024 || other_cap > 1024 || out_cap == 0)
    return CRDT_EINVAL;
  if (n_obj && (!d_self_n || !d_self_clk || !d_self_val || !d_other_n || !d_other_clk || !d_other_val || !d_out_n ||
                !d_out_clk || !d_out_val))
    return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_mvreg_merge(d_self_n, d_self_clk, d_self_val, self_cap, d_other_n, d_other_clk, d_other_val,
                            other_cap, d_out_n, d_out_clk, d_out_val, out_cap, n_obj, n_actors, ctx->d_status,
                            S(stream));
}

int crdt_mvreg_fold(crdt_ctx* ctx, const crdt_mvreg_view* h_reps, uint32_t n_reps, uint32_t* d_out_n,
                    uint64_t* d_out_clk, uint64_t* d_out_val, uint32_t out_cap, size_t n_obj, uint32_t n_actors,
                    void* stream) {
  if (!ctx || !h_reps || n_reps == 0 || n_reps > CRDT_MVREG_MAX_REPS || n_actors == 0 || out_cap == 0 ||
      out_cap > 2048)
    return CRDT_EINVAL;
  uint32_t total = 0;
  for (uint32_t r = 0; r < n_reps; ++r) {
    if (h_reps[r].cap == 0 || h_reps[r].cap > 1024) return CRDT_EINVAL;
    total += h_reps[r].cap;
  }
  if (total > 2048) return CRDT_EINVAL;
  if (n_obj) {
    if (!d_out_n || !d_out_clk || !d_out_val) return CRDT_EINVAL;
    for (uint32_t r = 0; r < n_reps; ++r) {
      if (!h_reps[r].n || !h_reps[r].clk || !h_reps[r].val) return CRDT_EINVAL;
      for (const void* w : {(const void*)d_out_n, (const void*)d_out_clk, (const void*)d_out_val})  // not in place
        if (w == h_reps[r].n || w == h_reps[r].clk || w == h_reps[r].val) return CRDT_EINVAL;
    }
  }
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_mvreg_fold(h_reps, n_reps, d_out_n, d_out_clk, d_out_val, out_cap, n_obj, n_actors, ctx->d_status,
                           S(stream));
}

static bool mvreg_op_caps_ok(uint32_t self_cap, uint32_t out_cap, uint32_t n_actors) {
  return n_actors && self_cap && self_cap <= 1024 && out_cap >= self_cap && out_cap <= 2048;
}

int crdt_mvreg_apply(crdt_ctx* ctx, const uint32_t* d_self_n, const uint64_t* d_self_clk, const uint64_t* d_self_val,
                     uint32_t self_cap, const crdt_mvreg_ops* ops, uint32_t* d_out_n, uint64_t* d_out_clk,
                     uint64_t* d_out_val, uint32_t out_cap, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || !ops || !mvreg_op_caps_ok(self_cap, out_cap, n_actors)) return CRDT_EINVAL;
  if (n_obj) {
    if (!d_self_n || !d_self_clk || !d_self_val || !d_out_n || !d_out_clk || !d_out_val || !ops->obj_end)
      return CRDT_EINVAL;
    if (d_out_n == d_self_n || d_out_clk == d_self_clk || d_out_val == d_self_val) return CRDT_EINVAL;  // not in place
  }
  if (ops->n_ops && (!ops->val || !ops->clk_end)) return CRDT_EINVAL;
  if (ops->n_clk && (!ops->clk_act || !ops->clk_ctr)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_mvreg_apply(d_self_n, d_self_clk, d_self_val, self_cap, *ops, d_out_n, d_out_clk, d_out_val, out_cap,
                            n_obj, n_actors, ctx->d_status, S(stream));
}

int crdt_mvreg_truncate(crdt_ctx* ctx, const uint32_t* d_self_n, const uint64_t* d_self_clk,
                        const uint64_t* d_self_val, uint32_t self_cap, const uint64_t* d_clock, uint32_t* d_out_n,
                        uint64_t* d_out_clk, uint64_t* d_out_val, uint32_t out_cap, size_t n_obj, uint32_t n_actors,
                        void* stream) {
  if (!ctx || !mvreg_op_caps_ok(self_cap, out_cap, n_actors)) return CRDT_EINVAL;
  if (n_obj) {
    if (!d_self_n || !d_self_clk || !d_self_val || !d_clock || !d_out_n || !d_out_clk || !d_out_val)
      return CRDT_EINVAL;
    if (d_out_n == d_self_n || d_out_clk == d_self_clk || d_out_val == d_self_val) return CRDT_EINVAL;  // not in place
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_mvreg_truncate(d_self_n, d_self_clk, d_self_val, self_cap, d_clock, d_out_n, d_out_clk, d_out_val,
                               out_cap, n_obj, n_actors, ctx->d_status, S(stream));
}

int crdt_mvreg_read_clock(crdt_ctx* ctx, const uint32_t* d_n, const uint64_t* d_clk, uint32_t cap,
                          uint64_t* d_out_clock, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || n_actors == 0 || cap == 0) return CRDT_EINVAL;
  if (n_obj && (!d_n || !d_clk || !d_out_clock || d_out_clock == d_clk)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_mvreg_read_clock(d_n, d_clk, cap, d_out_clock, n_obj, n_actors, ctx->d_status, S(stream));
}

// ---------------------------------------------------------------- the three Map types
// Their argument checks, in terms of map_limits.h: a slab's capacities are
// non-zero and within f times the side limits (f = 1: a merge's input, self of
// apply / truncate, an ingest's slab; f = kMapOutFactor: what a merge or an
// apply can leave, which egest reads); out of apply / truncate is additionally
// no smaller than self.
static bool map_actors_ok(uint32_t n_actors) { return n_actors != 0 && n_actors <= kMapActorsMax; }
static bool cap_ok(uint32_t cap, uint32_t limit) { return cap != 0 && cap <= limit; }

static bool caps_ok(const crdt_map_mvreg_slab* x, uint32_t f) {
  return cap_ok(x->kcap, kMapMvregKcap * f) && cap_ok(x->mcap, kMapMvregMcap * f) &&
         cap_ok(x->dcap, kMapMvregDcap * f) && cap_ok(x->scap, kMapMvregScap * f);
}
static bool caps_ok(const crdt_map_orswot_slab* x, uint32_t f) {
  return cap_ok(x->kcap, kMapOrswotKcap * f) && cap_ok(x->mcap, kMapOrswotMcap * f) &&
         cap_ok(x->vdcap, kMapOrswotVdcap * f) && cap_ok(x->vscap, kMapOrswotVscap * f) &&
         cap_ok(x->dcap, kMapOrswotDcap * f) && cap_ok(x->scap, kMapOrswotScap * f);
}
static bool caps_ok(const crdt_map_map_slab* x, uint32_t f) {
  return cap_ok(x->kcap, kMapMapKcap * f) && cap_ok(x->dcap, kMapMapDcap * f) && cap_ok(x->scap, kMapMapScap * f) &&
         caps_ok(&x->inner, f);
}
static bool out_caps_ok(const crdt_map_mvreg_slab* self, const crdt_map_mvreg_slab* out) {
  return caps_ok(out, kMapOutFactor) && out->kcap >= self->kcap && out->mcap >= self->mcap &&
         out->dcap >= self->dcap && out->scap >= self->scap;
}
static bool out_caps_ok(const crdt_map_orswot_slab* self, const crdt_map_orswot_slab* out) {
  return caps_ok(out, kMapOutFactor) && out->kcap >= self->kcap && out->mcap >= self->mcap &&
         out->vdcap >= self->vdcap && out->vscap >= self->vscap && out->dcap >= self->dcap && out->scap >= self->scap;
}
static bool out_caps_ok(const crdt_map_map_slab* self, const crdt_map_map_slab* out) {
  return caps_ok(out, kMapOutFactor) && out->kcap >= self->kcap && out->dcap >= self->dcap &&
         out->scap >= self->scap && out_caps_ok(&self->inner, &out->inner);
}
static bool ptrs_ok(const crdt_map_mvreg_slab* x) {
  return x->clock && x->n_keys && x->keys && x->eclock && x->mv_n && x->mv_clock && x->mv_val && x->n_def && x->dclock &&
         x->dset_n && x->dset;
}
static bool ptrs_ok(const crdt_map_orswot_slab* x) {
  return x->clock && x->n_keys && x->keys && x->eclock && x->vclock && x->vn_mem && x->vmem && x->vmclock &&
         x->vn_def && x->vdclock && x->vdset_n && x->vdset && x->n_def && x->dclock && x->dset_n && x->dset;
}
static bool ptrs_ok(const crdt_map_map_slab* x) {
  return x->clock && x->n_keys && x->keys && x->eclock && x->n_def && x->dclock && x->dset_n && x->dset &&
         ptrs_ok(&x->inner);
}

int crdt_map_mvreg_merge(crdt_ctx* ctx, const crdt_map_mvreg_slab* self, const crdt_map_mvreg_slab* other,
                         const crdt_map_mvreg_slab* out, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || !self || !other || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !caps_ok(other, 1u)) return CRDT_EINVAL;
  if (out->kcap < self->kcap + other->kcap || out->mcap < self->mcap + other->mcap ||
      out->dcap < self->dcap + other->dcap || out->scap < self->scap + other->scap)
    return CRDT_EINVAL;
  if (n_obj && (!ptrs_ok(self) || !ptrs_ok(other) || !ptrs_ok(out))) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_mvreg_merge(*self, *other, *out, n_obj, n_actors, ctx->d_status, ctx->d_ctl, S(stream),
                                ctx->variant);
}

int crdt_map_mvreg_apply(crdt_ctx* ctx, const crdt_map_mvreg_slab* self, const crdt_map_mvreg_ops* ops,
                         const crdt_map_mvreg_slab* out, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || !self || !ops || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !out_caps_ok(self, out)) return CRDT_EINVAL;
  if (n_obj) {
    if (!ptrs_ok(self) || !ptrs_ok(out) || !ops->obj_end) return CRDT_EINVAL;
    if (out->clock == self->clock) return CRDT_EINVAL;  // not in place
  }
  if (ops->n_ops && (!ops->kind || !ops->key || !ops->actor || !ops->counter || !ops->val || !ops->clk_end))
    return CRDT_EINVAL;
  if (ops->n_clk && (!ops->clk_act || !ops->clk_ctr)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_mvreg_apply(*self, *ops, *out, n_obj, n_actors, ctx->d_status, ctx->d_ctl, S(stream));
}

size_t crdt_map_map_merge_scratch_bytes(const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors) {
  return out ? map_map_scratch_bytes(*out, n_obj, n_actors) : 0u;
}

int crdt_map_map_merge(crdt_ctx* ctx, const crdt_map_map_slab* self, const crdt_map_map_slab* other,
                       const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors, void* d_scratch,
                       size_t scratch_bytes, void* stream) {
  if (!ctx || !self || !other || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !caps_ok(other, 1u)) return CRDT_EINVAL;
  const crdt_map_mvreg_slab &si = self->inner, &oi = other->inner, &ri = out->inner;
  if (out->kcap < self->kcap + other->kcap || out->dcap < self->dcap + other->dcap ||
      out->scap < self->scap + other->scap || ri.kcap < si.kcap + oi.kcap || ri.mcap < si.mcap + oi.mcap ||
      ri.dcap < si.dcap + oi.dcap || ri.scap < si.scap + oi.scap)
    return CRDT_EINVAL;
  if (n_obj) {
    if (!ptrs_ok(self) || !ptrs_ok(other) || !ptrs_ok(out)) return CRDT_EINVAL;
    if (!d_scratch || scratch_bytes < map_map_scratch_bytes(*out, n_obj, n_actors) || ((uintptr_t)d_scratch & 15u))
      return CRDT_EINVAL;
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_map_merge(*self, *other, *out, n_obj, n_actors, (uint8_t*)d_scratch, ctx->d_status, ctx->d_ctl,
                              S(stream));
}

size_t crdt_map_map_apply_scratch_bytes(const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors) {
  return out ? map_map_apply_scratch_bytes(*out, n_obj, n_actors) : 0u;
}

int crdt_map_map_apply(crdt_ctx* ctx, const crdt_map_map_slab* self, const crdt_map_map_ops* ops,
                       const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors, void* d_scratch,
                       size_t scratch_bytes, void* stream) {
  if (!ctx || !self || !ops || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !out_caps_ok(self, out)) return CRDT_EINVAL;
  if (n_obj) {
    if (!ptrs_ok(self) || !ptrs_ok(out) || !ops->obj_end) return CRDT_EINVAL;
    if (out->clock == self->clock || out->inner.clock == self->inner.clock) return CRDT_EINVAL;  // not in place
    if (!d_scratch || ((uintptr_t)d_scratch & 15u) ||
        scratch_bytes < map_map_apply_scratch_bytes(*out, n_obj, n_actors))
      return CRDT_EINVAL;
  }
  if (ops->n_ops && (!ops->kind || !ops->key || !ops->actor || !ops->counter || !ops->key2 || !ops->actor2 ||
                     !ops->counter2 || !ops->val || !ops->clk_end))
    return CRDT_EINVAL;
  if (ops->n_clk && (!ops->clk_act || !ops->clk_ctr)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_map_apply(*self, *ops, *out, n_obj, n_actors, (uint8_t*)d_scratch, ctx->d_status, ctx->d_ctl,
                              S(stream));
}

int crdt_map_orswot_merge(crdt_ctx* ctx, const crdt_map_orswot_slab* self, const crdt_map_orswot_slab* other,
                          const crdt_map_orswot_slab* out, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || !self || !other || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !caps_ok(other, 1u)) return CRDT_EINVAL;
  // (unlike apply and truncate, and unlike the other two merges, this entry
  // point only asks for non-zero out capacities: the kernel reports a row
  // that does not fit as CRDT_ECAPACITY. Kept as it is.)
  if (out->kcap == 0 || out->mcap == 0 || out->vdcap == 0 || out->vscap == 0 || out->dcap == 0 || out->scap == 0)
    return CRDT_EINVAL;
  if (map_orswot_lds_bytes(*self, *other, n_actors) > 65536) return CRDT_EINVAL;  // the kernel's workspace
  if (n_obj && (!ptrs_ok(self) || !ptrs_ok(other) || !ptrs_ok(out))) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_orswot_merge(*self, *other, *out, n_obj, n_actors, ctx->d_status, ctx->d_ctl, S(stream),
                                 ctx->variant);
}

int crdt_map_orswot_apply(crdt_ctx* ctx, const crdt_map_orswot_slab* self, const crdt_map_orswot_ops* ops,
                          const crdt_map_orswot_slab* out, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || !self || !ops || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !out_caps_ok(self, out)) return CRDT_EINVAL;
  if (map_orswot_apply_lds_bytes(*out, n_actors) > kMapOrswotApplyLdsMax) return CRDT_EINVAL;  // the kernel's workspace
  if (n_obj) {
    if (!ptrs_ok(self) || !ptrs_ok(out) || !ops->obj_end) return CRDT_EINVAL;
    if (out->clock == self->clock) return CRDT_EINVAL;  // not in place
  }
  if (ops->n_ops && (!ops->kind || !ops->key || !ops->actor || !ops->counter || !ops->member || !ops->clk_end))
    return CRDT_EINVAL;
  if (ops->n_clk && (!ops->clk_act || !ops->clk_ctr)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_orswot_apply(*self, *ops, *out, n_obj, n_actors, ctx->d_status, ctx->d_ctl, S(stream));
}

int crdt_map_mvreg_truncate(crdt_ctx* ctx, const crdt_map_mvreg_slab* self, const uint64_t* d_clock,
                            const crdt_map_mvreg_slab* out, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || !self || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !out_caps_ok(self, out)) return CRDT_EINVAL;
  if (n_obj) {
    if (!d_clock || !ptrs_ok(self) || !ptrs_ok(out)) return CRDT_EINVAL;
    if (out->clock == self->clock) return CRDT_EINVAL;  // not in place
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_mvreg_truncate(*self, d_clock, *out, n_obj, n_actors, ctx->d_status, ctx->d_ctl, S(stream));
}

int crdt_map_orswot_truncate(crdt_ctx* ctx, const crdt_map_orswot_slab* self, const uint64_t* d_clock,
                             const crdt_map_orswot_slab* out, size_t n_obj, uint32_t n_actors, void* stream) {
  if (!ctx || !self || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !out_caps_ok(self, out)) return CRDT_EINVAL;
  // the kernel's workspace: one nested set of self's capacities
  if (map_orswot_apply_lds_bytes(*self, n_actors) > kMapOrswotApplyLdsMax) return CRDT_EINVAL;
  if (n_obj) {
    if (!d_clock || !ptrs_ok(self) || !ptrs_ok(out)) return CRDT_EINVAL;
    if (out->clock == self->clock) return CRDT_EINVAL;  // not in place
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_orswot_truncate(*self, d_clock, *out, n_obj, n_actors, ctx->d_status, ctx->d_ctl, S(stream));
}

size_t crdt_map_map_truncate_scratch_bytes(const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors) {
  return out ? map_map_truncate_scratch_bytes(*out, n_obj, n_actors) : 0u;
}

int crdt_map_map_truncate(crdt_ctx* ctx, const crdt_map_map_slab* self, const uint64_t* d_clock,
                          const crdt_map_map_slab* out, size_t n_obj, uint32_t n_actors, void* d_scratch,
                          size_t scratch_bytes, void* stream) {
  if (!ctx || !self || !out || !map_actors_ok(n_actors)) return CRDT_EINVAL;
  if (!caps_ok(self, 1u) || !out_caps_ok(self, out)) return CRDT_EINVAL;
  if (n_obj) {
    if (!d_clock || !ptrs_ok(self) || !ptrs_ok(out)) return CRDT_EINVAL;
    if (out->clock == self->clock || out->inner.clock == self->inner.clock) return CRDT_EINVAL;  // not in place
    if (!d_scratch || ((uintptr_t)d_scratch & 15u) ||
        scratch_bytes < map_map_truncate_scratch_bytes(*out, n_obj, n_actors))
      return CRDT_EINVAL;
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_map_truncate(*self, d_clock, *out, n_obj, n_actors, (uint8_t*)d_scratch, ctx->d_status,
                                 ctx->d_ctl, S(stream));
}

// ------------------------------------------- bincode codec, MVReg and Map<u64, MVReg>
// (the Map slabs: ingest fills one within the side limits; egest reads any
// slab a merge or an apply can leave, kMapOutFactor times them)

int crdt_mvreg_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                            const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t val_bytes,
                            uint32_t n_actors, uint32_t* d_out_n, uint64_t* d_out_clk, uint64_t* d_out_val,
                            uint32_t out_cap, void* stream) {
  if (!ctx || n_actors == 0 || !bc_width_ok(actor_bytes) || !bc_width_ok(val_bytes) || out_cap == 0 || out_cap > 1024)
    return CRDT_EINVAL;
  if (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !d_out_n || !d_out_clk || !d_out_val)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_mvreg_bincode_ingest(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, val_bytes,
                                     n_actors, d_out_n, d_out_clk, d_out_val, out_cap, ctx->d_status, S(stream));
}

int crdt_mvreg_bincode_sizes(crdt_ctx* ctx, const uint32_t* d_n, const uint64_t* d_clk, const uint64_t* d_val,
                             uint32_t cap, size_t n_obj, uint32_t n_actors, uint32_t actor_bytes, uint32_t val_bytes,
                             uint64_t* d_sizes, void* stream) {
  if (!ctx || n_actors == 0 || !bc_width_ok(actor_bytes) || !bc_width_ok(val_bytes) || cap == 0 || cap > 2048)
    return CRDT_EINVAL;
  if (n_obj && (!d_n || !d_clk || !d_val || !d_sizes)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_mvreg_bincode_egest(d_n, d_clk, d_val, cap, n_obj, n_actors, actor_bytes, val_bytes, d_sizes, nullptr,
                                    nullptr, 0, ctx->d_status, S(stream));
}

int crdt_mvreg_to_bincode(crdt_ctx* ctx, const uint32_t* d_n, const uint64_t* d_clk, const uint64_t* d_val,
                          uint32_t cap, size_t n_obj, uint32_t n_actors, uint32_t actor_bytes, uint32_t val_bytes,
                          uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes, void* stream) {
  if (!ctx || n_actors == 0 || !bc_width_ok(actor_bytes) || !bc_width_ok(val_bytes) || cap == 0 || cap > 2048)
    return CRDT_EINVAL;
  if (n_obj && (!d_n || !d_clk || !d_val || !d_out || !d_out_off)) return CRDT_EINVAL;
  if (n_obj && out_bytes < 8u) return CRDT_EINVAL;  // the smallest blob (an empty register) is 8 bytes
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_mvreg_bincode_egest(d_n, d_clk, d_val, cap, n_obj, n_actors, actor_bytes, val_bytes, nullptr, d_out,
                                    d_out_off, out_bytes, ctx->d_status, S(stream));
}

int crdt_map_mvreg_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                                const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t key_bytes,
                                uint32_t val_bytes, uint32_t n_actors, const crdt_map_mvreg_slab* out, void* stream) {
  if (!ctx || !out || !map_actors_ok(n_actors) || !bc_width_ok(actor_bytes) || !bc_width_ok(key_bytes) ||
      !bc_width_ok(val_bytes) || !caps_ok(out, 1u))
    return CRDT_EINVAL;
  if (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !ptrs_ok(out))) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_bincode_ingest(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, key_bytes,
                                   val_bytes, n_actors, *out, ctx->d_status, S(stream));
}

int crdt_map_mvreg_bincode_sizes(crdt_ctx* ctx, const crdt_map_mvreg_slab* slab, size_t n_obj, uint32_t n_actors,
                                 uint32_t actor_bytes, uint32_t key_bytes, uint32_t val_bytes, uint64_t* d_sizes,
                                 void* stream) {
  if (!ctx || !slab || !map_actors_ok(n_actors) || !bc_width_ok(actor_bytes) || !bc_width_ok(key_bytes) ||
      !bc_width_ok(val_bytes) || !caps_ok(slab, kMapOutFactor))
    return CRDT_EINVAL;
  if (n_obj && (!ptrs_ok(slab) || !d_sizes)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_bincode_egest(*slab, n_obj, n_actors, actor_bytes, key_bytes, val_bytes, d_sizes, nullptr, nullptr,
                                  0, ctx->d_status, S(stream));
}

int crdt_map_mvreg_to_bincode(crdt_ctx* ctx, const crdt_map_mvreg_slab* slab, size_t n_obj, uint32_t n_actors,
                              uint32_t actor_bytes, uint32_t key_bytes, uint32_t val_bytes, uint8_t* d_out,
                              const uint64_t* d_out_off, size_t out_bytes, void* stream) {
  if (!ctx || !slab || !map_actors_ok(n_actors) || !bc_width_ok(actor_bytes) || !bc_width_ok(key_bytes) ||
      !bc_width_ok(val_bytes) || !caps_ok(slab, kMapOutFactor))
    return CRDT_EINVAL;
  if (n_obj && (!ptrs_ok(slab) || !d_out || !d_out_off)) return CRDT_EINVAL;
  if (n_obj && out_bytes < 24u) return CRDT_EINVAL;  // the smallest blob (the empty map) is 24 bytes
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_bincode_egest(*slab, n_obj, n_actors, actor_bytes, key_bytes, val_bytes, nullptr, d_out, d_out_off,
                                  out_bytes, ctx->d_status, S(stream));
}

// ------------------------------------ bincode codec, Map<u64, Orswot> and the nested map
// ingest: the side limits (the Map<u64, Orswot> merge's workspace rule is the
// merge's own); egest: kMapOutFactor times them
static bool bc_widths_ok(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return bc_width_ok(a) && bc_width_ok(b) && bc_width_ok(c) && bc_width_ok(d);
}

int crdt_map_orswot_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes,
                                 const uint64_t* d_blob_off, const uint64_t* d_blob_len, size_t n_obj,
                                 uint32_t actor_bytes, uint32_t key_bytes, uint32_t member_bytes, uint32_t n_actors,
                                 const crdt_map_orswot_slab* out, void* stream) {
  if (!ctx || !out || !map_actors_ok(n_actors) || !bc_widths_ok(actor_bytes, key_bytes, member_bytes, 1u) ||
      !caps_ok(out, 1u))
    return CRDT_EINVAL;
  if (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !ptrs_ok(out))) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_orswot_bincode_ingest(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, key_bytes,
                                          member_bytes, n_actors, *out, ctx->d_status, S(stream));
}

int crdt_map_orswot_bincode_sizes(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, size_t n_obj, uint32_t n_actors,
                                  uint32_t actor_bytes, uint32_t key_bytes, uint32_t member_bytes, uint64_t* d_sizes,
                                  void* stream) {
  if (!ctx || !slab || !map_actors_ok(n_actors) || !bc_widths_ok(actor_bytes, key_bytes, member_bytes, 1u) ||
      !caps_ok(slab, kMapOutFactor))
    return CRDT_EINVAL;
  if (n_obj && (!ptrs_ok(slab) || !d_sizes)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_orswot_bincode_egest(*slab, n_obj, n_actors, actor_bytes, key_bytes, member_bytes, d_sizes,
                                         nullptr, nullptr, 0, ctx->d_status, S(stream));
}

int crdt_map_orswot_to_bincode(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, size_t n_obj, uint32_t n_actors,
                               uint32_t actor_bytes, uint32_t key_bytes, uint32_t member_bytes, uint8_t* d_out,
                               const uint64_t* d_out_off, size_t out_bytes, void* stream) {
  if (!ctx || !slab || !map_actors_ok(n_actors) || !bc_widths_ok(actor_bytes, key_bytes, member_bytes, 1u) ||
      !caps_ok(slab, kMapOutFactor))
    return CRDT_EINVAL;
  if (n_obj && (!ptrs_ok(slab) || !d_out || !d_out_off)) return CRDT_EINVAL;
  if (n_obj && out_bytes < 24u) return CRDT_EINVAL;  // the smallest blob (the empty map) is 24 bytes
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_orswot_bincode_egest(*slab, n_obj, n_actors, actor_bytes, key_bytes, member_bytes, nullptr, d_out,
                                         d_out_off, out_bytes, ctx->d_status, S(stream));
}

int crdt_map_map_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                              const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t key_bytes,
                              uint32_t inner_key_bytes, uint32_t val_bytes, uint32_t n_actors,
                              const crdt_map_map_slab* out, void* stream) {
  if (!ctx || !out || !map_actors_ok(n_actors) ||
      !bc_widths_ok(actor_bytes, key_bytes, inner_key_bytes, val_bytes) || !caps_ok(out, 1u))
    return CRDT_EINVAL;
  if (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !ptrs_ok(out))) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_map_bincode_ingest(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, key_bytes,
                                       inner_key_bytes, val_bytes, n_actors, *out, ctx->d_status, S(stream));
}

int crdt_map_map_bincode_sizes(crdt_ctx* ctx, const crdt_map_map_slab* slab, size_t n_obj, uint32_t n_actors,
                               uint32_t actor_bytes, uint32_t key_bytes, uint32_t inner_key_bytes, uint32_t val_bytes,
                               uint64_t* d_sizes, void* stream) {
  if (!ctx || !slab || !map_actors_ok(n_actors) ||
      !bc_widths_ok(actor_bytes, key_bytes, inner_key_bytes, val_bytes) || !caps_ok(slab, kMapOutFactor))
    return CRDT_EINVAL;
  if (n_obj && (!ptrs_ok(slab) || !d_sizes)) return CRDT_EINVAL;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_map_bincode_egest(*slab, n_obj, n_actors, actor_bytes, key_bytes, inner_key_bytes, val_bytes,
                                      d_sizes, nullptr, nullptr, 0, ctx->d_status, S(stream));
}

int crdt_map_map_to_bincode(crdt_ctx* ctx, const crdt_map_map_slab* slab, size_t n_obj, uint32_t n_actors,
                            uint32_t actor_bytes, uint32_t key_bytes, uint32_t inner_key_bytes, uint32_t val_bytes,
                            uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes, void* stream) {
  if (!ctx || !slab || !map_actors_ok(n_actors) ||
      !bc_widths_ok(actor_bytes, key_bytes, inner_key_bytes, val_bytes) || !caps_ok(slab, kMapOutFactor))
    return CRDT_EINVAL;
  if (n_obj && (!ptrs_ok(slab) || !d_out || !d_out_off)) return CRDT_EINVAL;
  if (n_obj && out_bytes < 24u) return CRDT_EINVAL;  // the smallest blob (the empty map) is 24 bytes
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_map_bincode_egest(*slab, n_obj, n_actors, actor_bytes, key_bytes, inner_key_bytes, val_bytes,
                                      nullptr, d_out, d_out_off, out_bytes, ctx->d_status, S(stream));
}

// ---------------------------------------------------------------- the read path
namespace {
constexpr uint32_t kReadKcapMax = kMapOutFactor * kMapMvregKcap;  // the three slabs' output kcap limit
static_assert(kMapOrswotKcap == kMapMvregKcap && kMapMapKcap == kMapMvregKcap, "one kcap limit for the view");

bool read_queries_ok(const crdt_read_queries* q, size_t n_obj) {
  return q && !(n_obj && !q->obj_end) && !(q->n_q && (!q->kind || !q->key));
}
// Is a (non-null) output array w one of the input arrays?
bool read_alias(const void* w, const crdt_read_queries* q, std::initializer_list<const void*> state) {
  if (!w) return false;
  for (const void* r : {(const void*)q->obj_end, (const void*)q->kind, (const void*)q->key, (const void*)q->actor})
    if (w == r) return true;
  for (const void* r : state)
    if (w == r) return true;
  return false;
}
bool read_sizes_alias(const crdt_read_sizes* z, const crdt_read_queries* q, std::initializer_list<const void*> state) {
  for (const void* w : {(const void*)z->val, (const void*)z->slot, (const void*)z->dot_ctr, (const void*)z->add_len,
                        (const void*)z->rm_len, (const void*)z->list_len})
    if (read_alias(w, q, state)) return true;
  return false;
}
// The write call's groups: a wanted group has all its arrays (with queries to
// write), and no output is an input (the *_end arrays are inputs too).
bool read_out_ok(const crdt_read_out* o, const crdt_read_queries* q, std::initializer_list<const void*> state) {
  if (q->n_q) {
    if (o->add_end && o->n_add && (!o->add_act || !o->add_ctr)) return false;
    if (o->rm_end && o->n_rm && (!o->rm_act || !o->rm_ctr)) return false;
    if (o->list_end && o->n_list && !o->list_key) return false;
  }
  for (const void* w : {(const void*)o->add_act, (const void*)o->add_ctr, (const void*)o->rm_act,
                        (const void*)o->rm_ctr, (const void*)o->list_key}) {
    if (read_alias(w, q, state)) return false;
    if (w && (w == o->add_end || w == o->rm_end || w == o->list_end)) return false;
  }
  return true;
}
int orswot_read(crdt_ctx* ctx, const crdt_orswot_batch* b, const crdt_read_queries* q, uint32_t n_actors,
                uint32_t flags, const crdt_read_sizes* sizes, const crdt_read_out* out, bool write, void* stream) {
  if (!ctx || !b || (write ? !out : !sizes) || n_actors == 0 || (flags & ~CRDT_ORSWOT_SPARSE_CLOCK) ||
      !read_queries_ok(q, b->n_obj))
    return CRDT_EINVAL;
  if (b->n_obj && (!b->base || !b->off)) return CRDT_EINVAL;
  const std::initializer_list<const void*> state = {b->base, b->off};
  if (write ? !read_out_ok(out, q, state) : read_sizes_alias(sizes, q, state)) return CRDT_EINVAL;
  if (b->n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_orswot_read(*b, *q, n_actors, flags, sizes, out, ctx->d_status, S(stream));
}
int map_read(crdt_ctx* ctx, const crdt_map_read_view* v, const crdt_read_queries* q, size_t n_obj, uint32_t n_actors,
             const crdt_read_sizes* sizes, const crdt_read_out* out, bool write, void* stream) {
  if (!ctx || !v || (write ? !out : !sizes) || !map_actors_ok(n_actors) || !cap_ok(v->kcap, kReadKcapMax) ||
      !read_queries_ok(q, n_obj))
    return CRDT_EINVAL;
  if (n_obj && (!v->clock || !v->n_keys || !v->keys || !v->eclock)) return CRDT_EINVAL;
  const std::initializer_list<const void*> state = {v->clock, v->n_keys, v->keys, v->eclock};
  if (write ? !read_out_ok(out, q, state) : read_sizes_alias(sizes, q, state)) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_read(*v, *q, n_obj, n_actors, sizes, out, ctx->d_status, S(stream));
}
}  // namespace

int crdt_orswot_read_sizes(crdt_ctx* ctx, const crdt_orswot_batch* batch, const crdt_read_queries* queries,
                           uint32_t n_actors, uint32_t flags, const crdt_read_sizes* sizes, void* stream) {
  return orswot_read(ctx, batch, queries, n_actors, flags, sizes, nullptr, false, stream);
}
int crdt_orswot_read(crdt_ctx* ctx, const crdt_orswot_batch* batch, const crdt_read_queries* queries,
                     uint32_t n_actors, uint32_t flags, const crdt_read_out* out, void* stream) {
  return orswot_read(ctx, batch, queries, n_actors, flags, nullptr, out, true, stream);
}
int crdt_map_read_sizes(crdt_ctx* ctx, const crdt_map_read_view* view, const crdt_read_queries* queries,
                        size_t n_obj, uint32_t n_actors, const crdt_read_sizes* sizes, void* stream) {
  return map_read(ctx, view, queries, n_obj, n_actors, sizes, nullptr, false, stream);
}
int crdt_map_read(crdt_ctx* ctx, const crdt_map_read_view* view, const crdt_read_queries* queries, size_t n_obj,
                  uint32_t n_actors, const crdt_read_out* out, void* stream) {
  return map_read(ctx, view, queries, n_obj, n_actors, nullptr, out, true, stream);
}
int crdt_map_mvreg_get(crdt_ctx* ctx, const crdt_map_mvreg_slab* slab, const crdt_read_queries* queries,
                       size_t n_obj, uint32_t n_actors, uint32_t* d_out_n, uint64_t* d_out_clk,
                       uint64_t* d_out_val, uint32_t out_cap, void* stream) {
  if (!ctx || !slab || !map_actors_ok(n_actors) || !cap_ok(slab->kcap, kReadKcapMax) ||
      !cap_ok(slab->mcap, kMapOutFactor * kMapMvregMcap) || out_cap < slab->mcap || !read_queries_ok(queries, n_obj))
    return CRDT_EINVAL;
  if (n_obj && (!slab->n_keys || !slab->keys || !slab->mv_n || !slab->mv_clock || !slab->mv_val)) return CRDT_EINVAL;
  if (n_obj && queries->n_q && (!d_out_n || !d_out_clk || !d_out_val)) return CRDT_EINVAL;
  for (const void* w : {(const void*)d_out_n, (const void*)d_out_clk, (const void*)d_out_val})
    if (read_alias(w, queries, {slab->n_keys, slab->keys, slab->mv_n, slab->mv_clock, slab->mv_val}))
      return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_mvreg_get(*slab, *queries, n_obj, n_actors, d_out_n, d_out_clk, d_out_val, out_cap,
                              ctx->d_status, S(stream));
}

namespace {
int map_orswot_get(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, const crdt_read_queries* q, size_t n_obj,
                   uint32_t n_actors, uint64_t* d_sizes, uint32_t* d_present, uint8_t* d_out,
                   const uint64_t* d_out_off, size_t out_bytes, bool write, void* stream) {
  if (!ctx || !slab || !map_actors_ok(n_actors) || !cap_ok(slab->kcap, kReadKcapMax) || !read_queries_ok(q, n_obj))
    return CRDT_EINVAL;
  // what the get reads: the key search's arrays and the nested Orswots
  const std::initializer_list<const void*> state = {slab->n_keys, slab->keys,    slab->vclock,  slab->vn_mem,
                                                    slab->vmem,   slab->vmclock, slab->vn_def,  slab->vdclock,
                                                    slab->vdset_n, slab->vdset};
  if (n_obj)
    for (const void* r : state)
      if (!r) return CRDT_EINVAL;
  if (q->n_q && (write ? (!d_out_off || (n_obj && !d_out)) : !d_sizes)) return CRDT_EINVAL;
  for (const void* w : {(const void*)d_sizes, (const void*)d_present, (const void*)d_out})
    if (read_alias(w, q, state) || (w && w == (const void*)d_out_off)) return CRDT_EINVAL;
  if (d_out_off && read_alias(d_out_off, q, {})) return CRDT_EINVAL;
  if (d_sizes && (const void*)d_sizes == (const void*)d_present) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_orswot_get(*slab, *q, n_obj, n_actors, d_sizes, d_present, d_out, d_out_off, out_bytes,
                               ctx->d_status, S(stream));
}
}  // namespace

int crdt_map_orswot_get_sizes(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, const crdt_read_queries* queries,
                              size_t n_obj, uint32_t n_actors, uint64_t* d_sizes, uint32_t* d_present, void* stream) {
  return map_orswot_get(ctx, slab, queries, n_obj, n_actors, d_sizes, d_present, nullptr, nullptr, 0, false, stream);
}
int crdt_map_orswot_get(crdt_ctx* ctx, const crdt_map_orswot_slab* slab, const crdt_read_queries* queries,
                        size_t n_obj, uint32_t n_actors, uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes,
                        void* stream) {
  return map_orswot_get(ctx, slab, queries, n_obj, n_actors, nullptr, nullptr, d_out, d_out_off, out_bytes, true,
                        stream);
}
int crdt_map_map_get(crdt_ctx* ctx, const crdt_map_map_slab* slab, const crdt_read_queries* queries, size_t n_obj,
                     uint32_t n_actors, const crdt_map_mvreg_slab* out, uint32_t* d_present, void* stream) {
  if (!ctx || !slab || !out || !map_actors_ok(n_actors) || !cap_ok(slab->kcap, kReadKcapMax) ||
      !read_queries_ok(queries, n_obj))
    return CRDT_EINVAL;
  const crdt_map_mvreg_slab* in = &slab->inner;
  if (in->kcap == 0 || out->kcap < in->kcap || out->mcap < in->mcap || out->dcap < in->dcap || out->scap < in->scap)
    return CRDT_EINVAL;
  if (n_obj && (!slab->n_keys || !slab->keys || !ptrs_ok(in))) return CRDT_EINVAL;
  if (n_obj && queries->n_q && !ptrs_ok(out)) return CRDT_EINVAL;
  const std::initializer_list<const void*> state = {slab->n_keys, slab->keys,     in->clock, in->n_keys,
                                                    in->keys,     in->eclock,     in->mv_n,  in->mv_clock,
                                                    in->mv_val,   in->n_def,      in->dclock, in->dset_n,
                                                    in->dset};
  for (const void* w : {(const void*)out->clock, (const void*)out->n_keys, (const void*)out->keys,
                        (const void*)out->eclock, (const void*)out->mv_n, (const void*)out->mv_clock,
                        (const void*)out->mv_val, (const void*)out->n_def, (const void*)out->dclock,
                        (const void*)out->dset_n, (const void*)out->dset, (const void*)d_present})
    if (read_alias(w, queries, state)) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_map_map_get(*slab, *queries, n_obj, n_actors, *out, d_present, ctx->d_status, S(stream));
}

// ------------------------------------------------------------------------
// bincode of the Orswot, MVReg and Map ops (ops_bincode.hip)
namespace {
// What an op type uses: the four widths and the eight per-op field arrays, in
// the order of crdt_op_widths / crdt_op_arrays (clk_end and the pair arrays
// are every type's).
struct OpUse {
  bool width[4];  // actor, key, key2, val
  bool field[8];  // kind, key, actor, counter, key2, actor2, counter2, val
};
OpUse op_use(uint32_t op_type) {
  switch (op_type) {
    case CRDT_OPS_ORSWOT: return {{true, false, true, false}, {true, false, true, true, true, false, false, false}};
    case CRDT_OPS_MVREG: return {{true, false, false, true}, {false, false, false, false, false, false, false, true}};
    case CRDT_OPS_MAP_MVREG: return {{true, true, false, true}, {true, true, true, true, false, false, false, true}};
    case CRDT_OPS_MAP_ORSWOT: return {{true, true, true, false}, {true, true, true, true, true, false, false, false}};
    default: return {{true, true, true, true}, {true, true, true, true, true, true, true, true}};
  }
}
bool op_width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }
// The widths the kernels take: the used ones checked, the others 8 (any value
// fits, nothing is read at them).
bool op_widths(uint32_t op_type, const crdt_op_widths* w, crdt_op_widths* norm) {
  if (!w || op_type > CRDT_OPS_MAP_MAP) return false;
  const OpUse u = op_use(op_type);
  const uint32_t in[4] = {w->actor_bytes, w->key_bytes, w->key2_bytes, w->val_bytes};
  uint32_t out[4];
  for (int k = 0; k < 4; ++k) {
    if (u.width[k] && !op_width_ok(in[k])) return false;
    out[k] = u.width[k] ? in[k] : 8u;
  }
  *norm = {out[0], out[1], out[2], out[3]};
  return true;
}
// The arrays the type uses are there (n_ops > 0), none of them (clk_end only
// with `with_end`: it is an input of the ingest) equals one of `others`.
bool op_arrays_ok(uint32_t op_type, const crdt_op_arrays* a, bool with_end, std::initializer_list<const void*> others) {
  const OpUse u = op_use(op_type);
  const void* f[8] = {a->kind, a->key, a->actor, a->counter, a->key2, a->actor2, a->counter2, a->val};
  std::vector<const void*> mine;
  for (int k = 0; k < 8; ++k)
    if (u.field[k]) mine.push_back(f[k]);
  if (!a->clk_end) return false;
  if (with_end) mine.push_back(a->clk_end);
  if (a->n_clk) {
    mine.push_back(a->clk_act);
    mine.push_back(a->clk_ctr);
  }
  for (const void* m : mine) {
    if (!m) return false;
    for (const void* o : others)
      if (o && o == m) return false;
  }
  return true;
}
}  // namespace

int crdt_ops_bincode_clk_lens(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                              const uint64_t* d_blob_len, size_t n_ops, uint32_t op_type, const crdt_op_widths* widths,
                              uint32_t* d_clk_len, void* stream) {
  crdt_op_widths W;
  if (!ctx || !op_widths(op_type, widths, &W)) return CRDT_EINVAL;
  if (n_ops && (!d_blobs || !d_blob_off || !d_blob_len || !d_clk_len)) return CRDT_EINVAL;
  if (n_ops && ((const void*)d_clk_len == d_blobs || (const void*)d_clk_len == d_blob_off ||
                (const void*)d_clk_len == d_blob_len))
    return CRDT_EINVAL;
  if (n_ops == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_ops_bincode_clk_lens(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_ops, op_type, W, d_clk_len,
                                     ctx->d_status, S(stream));
}

int crdt_ops_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                          const uint64_t* d_blob_len, uint32_t op_type, const crdt_op_widths* widths,
                          const crdt_op_arrays* out, uint32_t* d_op_err, void* stream) {
  crdt_op_widths W;
  if (!ctx || !out || !op_widths(op_type, widths, &W)) return CRDT_EINVAL;
  if (out->n_ops && (!d_blobs || !d_blob_off || !d_blob_len)) return CRDT_EINVAL;
  // clk_end is an input here: no output may be it, or a blob array
  if (out->n_ops && !op_arrays_ok(op_type, out, false, {d_blobs, d_blob_off, d_blob_len, out->clk_end}))
    return CRDT_EINVAL;
  if (out->n_ops && d_op_err)
    for (const void* r : {(const void*)d_blobs, (const void*)d_blob_off, (const void*)d_blob_len,
                          (const void*)out->clk_end})
      if (r == d_op_err) return CRDT_EINVAL;
  if (out->n_ops == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_ops_from_bincode(d_blobs, blob_bytes, d_blob_off, d_blob_len, op_type, W, *out, d_op_err,
                                 ctx->d_status, S(stream));
}

int crdt_ops_bincode_sizes(crdt_ctx* ctx, uint32_t op_type, const crdt_op_widths* widths, const crdt_op_arrays* ops,
                           uint64_t* d_sizes, void* stream) {
  crdt_op_widths W;
  if (!ctx || !ops || !op_widths(op_type, widths, &W)) return CRDT_EINVAL;
  if (ops->n_ops && (!d_sizes || !op_arrays_ok(op_type, ops, true, {d_sizes}))) return CRDT_EINVAL;
  if (ops->n_ops == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_ops_to_bincode(op_type, W, *ops, d_sizes, nullptr, nullptr, 0, ctx->d_status, S(stream));
}

int crdt_ops_to_bincode(crdt_ctx* ctx, uint32_t op_type, const crdt_op_widths* widths, const crdt_op_arrays* ops,
                        uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes, void* stream) {
  crdt_op_widths W;
  if (!ctx || !ops || !op_widths(op_type, widths, &W)) return CRDT_EINVAL;
  if (ops->n_ops && (!d_out || !d_out_off || (const void*)d_out == d_out_off ||
                     !op_arrays_ok(op_type, ops, true, {d_out})))
    return CRDT_EINVAL;
  if (ops->n_ops == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_ops_to_bincode(op_type, W, *ops, nullptr, d_out, d_out_off, out_bytes, ctx->d_status, S(stream));
}

}  // extern "C"
