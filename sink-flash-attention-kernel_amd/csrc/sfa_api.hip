// extern "C" entry points of libsfa.so (declared in include/sfa.h): argument
// validation, kernel-family choice, workspace carving.  No allocation, no sync.
#include <cmath>
#include <cstring>

#include "sfa_common.hpp"
#include "sfa_internal.hpp"

namespace sfa {

static thread_local char g_err[512] = "";
static char g_path[128] = "";  // diagnostic only: last kernel family dispatched in this process (any thread)

// measurement hook (sfa_debug_set_stage_events): process-global on purpose, the autograd thread runs sfa_bwd
void* g_debug_ptr = nullptr;
int g_variant[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // sfa_debug_set_variant: read by A/B builds (-DSFA_AB) only
static void* const* g_stage_events = nullptr;
static int g_stage_count = 0;
bool stage_events_armed() { return g_stage_events != nullptr; }
void record_stage(int i, hipStream_t stream) {
    if (g_stage_events && i < g_stage_count && g_stage_events[i]) (void)hipEventRecord((hipEvent_t)g_stage_events[i], stream);
}

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
void set_path(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_path, sizeof(g_path), fmt, ap);
    va_end(ap);
}

namespace {

int check_tensor(const sfa_tensor* t, const char* name) {
    SFA_CHECK_ARG(t != nullptr, "%s: null tensor descriptor", name);
    SFA_CHECK_ARG(t->dtype == SFA_DTYPE_F32 || t->dtype == SFA_DTYPE_F16 || t->dtype == SFA_DTYPE_BF16,
                  "%s: unknown dtype %d", name, t->dtype);
    for (int i = 0; i < 4; ++i) SFA_CHECK_ARG(t->shape[i] >= 0, "%s: negative shape[%d]", name, i);
    const bool empty = t->shape[0] == 0 || t->shape[1] == 0 || t->shape[2] == 0 || t->shape[3] == 0;
    SFA_CHECK_ARG(empty || t->ptr != nullptr, "%s: null data pointer", name);
    SFA_CHECK_ARG(t->shape[3] <= 1 || t->stride[3] == 1, "%s: last-dim stride must be 1 (got %lld)", name,
                  (long long)t->stride[3]);
    for (int i = 0; i < 3; ++i)
        SFA_CHECK_ARG(t->stride[i] >= 0, "%s: negative stride[%d] not supported", name, i);
    return SFA_OK;
}

int same_shape(const sfa_tensor* a, const sfa_tensor* b, const char* an, const char* bn) {
    for (int i = 0; i < 4; ++i)
        SFA_CHECK_ARG(a->shape[i] == b->shape[i], "%s and %s differ in shape[%d]: %lld vs %lld", an, bn, i,
                      (long long)a->shape[i], (long long)b->shape[i]);
    SFA_CHECK_ARG(a->dtype == b->dtype, "%s and %s differ in dtype", an, bn);
    return SFA_OK;
}

// shape contract of SinkFlashAttentionFunc.forward (sink_flash_attention.py:494-498)
int check_prefill(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, Problem* p, int num_sink,
                  int window, float scale) {
    int st;
    if ((st = check_tensor(q, "q")) || (st = check_tensor(k, "k")) || (st = check_tensor(v, "v"))) return st;
    if ((st = same_shape(k, v, "k", "v"))) return st;
    SFA_CHECK_ARG(q->dtype == k->dtype, "q and k differ in dtype");
    SFA_CHECK_ARG(q->shape[0] == k->shape[0], "batch mismatch: q %lld vs k %lld", (long long)q->shape[0],
                  (long long)k->shape[0]);
    // the reference needs N_q == N_kv; here the keys may outnumber the queries (the queries are then the LAST N_q
    // positions: chunked prefill, a sequence-parallel rank with its halo keys prepended)
    SFA_CHECK_ARG(q->shape[2] <= k->shape[2], "prefill needs N_q <= N_kv (q %lld, k %lld)", (long long)q->shape[2],
                  (long long)k->shape[2]);
    SFA_CHECK_ARG(q->shape[3] == k->shape[3], "head dim mismatch");
    SFA_CHECK_ARG(k->shape[1] > 0 && q->shape[1] % k->shape[1] == 0, "H_q (%lld) must be divisible by H_kv (%lld)",
                  (long long)q->shape[1], (long long)k->shape[1]);
    SFA_CHECK_ARG(q->shape[2] < (1ll << 30) && q->shape[0] * q->shape[1] < (1ll << 30), "problem too large");
    SFA_CHECK_ARG(num_sink >= 0, "num_sink must be >= 0");
    SFA_CHECK_ARG(std::isfinite(scale), "scale must be finite");
    p->B = (int)q->shape[0];
    p->Hq = (int)q->shape[1];
    p->Hkv = (int)k->shape[1];
    p->N = (int)q->shape[2];
    p->Nk = (int)k->shape[2];
    p->D = (int)q->shape[3];
    p->num_sink = num_sink;
    p->window = window;
    p->scale = scale;
    return SFA_OK;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct BwdWorkspace {
    size_t delta_off, dsaux_off, mfma_off, total;
};

BwdWorkspace bwd_layout(const Problem& p, int dtype, bool use_mfma, unsigned flags) {
    BwdWorkspace w;
    size_t off = 0;
    w.delta_off = off;
    off += align256((size_t)p.B * p.Hq * p.N * sizeof(float));
    w.dsaux_off = off;
    off += align256((size_t)p.B * p.Hq * (size_t)bwd_preprocess_nblk(p.N) * sizeof(float));
    w.mfma_off = off;
    if (use_mfma) off += align256(bwd_mfma_workspace_bytes(p, dtype, flags));
    w.total = off;
    return w;
}

}  // namespace
}  // namespace sfa

using namespace sfa;

extern "C" {

int sfa_abi_version(void) { return SFA_ABI_VERSION; }
const char* sfa_last_error(void) { return g_err; }
const char* sfa_last_path(void) { return g_path; }
int sfa_debug_set_variant(int which, int value) {
    if (which < 0 || which >= 8) return SFA_ERR_INVALID_ARGUMENT;
    __atomic_store_n(&sfa::g_variant[which], value, __ATOMIC_RELAXED);
    return SFA_OK;
}

int sfa_debug_set_ptr(void* p) {
    sfa::g_debug_ptr = p;
    return SFA_OK;
}

int sfa_debug_set_stage_events(void* const* events, int count) {
    g_stage_events = count > 0 ? events : nullptr;
    g_stage_count = count > 0 ? count : 0;
    return SFA_OK;
}

int sfa_fwd(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o, float* lse,
            const float* s_aux, int num_sink, int window, float scale, unsigned flags, void* stream) {
    g_err[0] = 0;
    Problem p;
    int st = check_prefill(q, k, v, &p, num_sink, window, scale);
    if (st) return st;
    if ((st = check_tensor(o, "o")) || (st = same_shape(q, o, "q", "o"))) return st;
    if (p.B == 0 || p.Hq == 0 || p.N == 0) return SFA_OK;
    SFA_CHECK_ARG(p.D > 0, "head dim must be > 0");
    SFA_CHECK_ARG(lse != nullptr, "lse: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & SFA_FLAG_FORCE_GENERIC) && fwd_mfma_supported(q->dtype, p.D))
        return fwd_mfma(q, k, v, o, lse, s_aux, p, s);
    if (p.Nk != p.N) {
        set_error("N_q != N_kv is served by the MFMA kernels only (16-bit dtypes, head dims 64/80/96/128)");
        return SFA_ERR_UNSUPPORTED;
    }
    return fwd_generic(q, k, v, o, lse, s_aux, p, s);
}

size_t sfa_bwd_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t N, int64_t D, int dtype, int num_sink,
                               int window, unsigned flags) {
    Problem p{(int)B, (int)Hq, (int)Hkv, (int)N, (int)D, num_sink, window, 1.f};
    const bool use_mfma = !(flags & SFA_FLAG_FORCE_GENERIC) && bwd_mfma_supported(dtype, (int)D);
    return bwd_layout(p, dtype, use_mfma, flags).total;
}

int sfa_bwd(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o,
            const sfa_tensor* d_o, const float* lse, const float* s_aux, const sfa_tensor* dq, const sfa_tensor* dk,
            const sfa_tensor* dv, float* ds_aux, void* workspace, size_t workspace_bytes, int num_sink, int window,
            float scale, unsigned flags, void* stream) {
    g_err[0] = 0;
    Problem p;
    int st = check_prefill(q, k, v, &p, num_sink, window, scale);
    if (st) return st;
    if ((st = check_tensor(o, "o")) || (st = same_shape(q, o, "q", "o"))) return st;
    if ((st = check_tensor(d_o, "do")) || (st = same_shape(q, d_o, "q", "do"))) return st;
    if ((st = check_tensor(dq, "dq")) || (st = same_shape(q, dq, "q", "dq"))) return st;
    if ((st = check_tensor(dk, "dk")) || (st = same_shape(k, dk, "k", "dk"))) return st;
    if ((st = check_tensor(dv, "dv")) || (st = same_shape(v, dv, "v", "dv"))) return st;
    if (p.B == 0 || p.Hq == 0 || p.N == 0) return SFA_OK;
    SFA_CHECK_ARG(p.D > 0, "head dim must be > 0");
    SFA_CHECK_ARG(lse != nullptr, "lse: null pointer");
    SFA_CHECK_ARG((s_aux == nullptr) == (ds_aux == nullptr), "ds_aux must be given iff s_aux is");
    const bool use_mfma = !(flags & SFA_FLAG_FORCE_GENERIC) && bwd_mfma_supported(q->dtype, p.D);
    if (use_mfma && (st = bwd_mfma_refused(q, k, v, d_o, dq, dk, dv, p))) return st;     // before the preprocess: nothing written
    const BwdWorkspace w = bwd_layout(p, q->dtype, use_mfma, flags);
    if (workspace == nullptr || workspace_bytes < w.total || ((uintptr_t)workspace & 255) != 0) {
        set_error("bwd workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", w.total, workspace_bytes,
                  workspace);
        return SFA_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    float* delta = reinterpret_cast<float*>((char*)workspace + w.delta_off);
    float* dsaux_part = reinterpret_cast<float*>((char*)workspace + w.dsaux_off);
    record_stage(0, s);
    // the row constants of the dK/dV kernel come out of the same pass whenever it is the vectorised one
    const bool fuse = use_mfma && bwd_mfma_wants_consts() && bwd_preprocess_vectorised(o, d_o, p);
    st = bwd_preprocess(o, d_o, lse, s_aux, delta, dsaux_part, ds_aux, p, s,
                        fuse ? reinterpret_cast<float*>((char*)workspace + w.mfma_off) : nullptr, bwd_mfma_lse_factor(p, flags));
    record_stage(1, s);
    if (st) return st;
    if (use_mfma)
        st = bwd_mfma(q, k, v, d_o, lse, delta, dq, dk, dv, (char*)workspace + w.mfma_off, p, flags, s, fuse);
    else if (p.Nk != p.N) {
        set_error("N_q != N_kv is served by the MFMA kernels only (16-bit dtypes, head dims 64/80/96/128)");
        st = SFA_ERR_UNSUPPORTED;
    } else
        st = bwd_generic(q, k, v, d_o, lse, delta, dq, dk, dv, p, s);
    record_stage(3, s);
    return st;
}

int sfa_varlen_supported(int dtype, int64_t D) {
    return fwd_mfma_supported(dtype, (int)D) && bwd_mfma_varlen_supported(dtype, (int)D) ? 1 : 0;
}

// shared checks of the packed entry points; on success *p describes the packed tensors (B = 1, N = total rows) and
// *run the launch (B = n_seq, N = max_seqlen, cu set)
static int check_varlen(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const int32_t* cu, int n_seq,
                        int max_seqlen, int num_sink, int window, float scale, Problem* p, Problem* run) {
    int st = check_prefill(q, k, v, p, num_sink, window, scale);
    if (st) return st;
    SFA_CHECK_ARG(p->B == 1, "packed layout: batch dim must be 1 (got %d)", p->B);
    SFA_CHECK_ARG(p->N == p->Nk, "packed layout: q and k must have the same number of rows");
    SFA_CHECK_ARG(cu != nullptr && n_seq >= 1, "cu_seqlens: need a device array of n_seq + 1 >= 2 offsets");
    SFA_CHECK_ARG(max_seqlen >= 1 && max_seqlen <= p->N, "max_seqlen %d out of range (total rows %d)", max_seqlen, p->N);
    if (!sfa_varlen_supported(q->dtype, p->D)) {
        set_error("packed (varlen) kernels exist for 16-bit dtypes and head dims 64/80/96/128 only");
        return SFA_ERR_UNSUPPORTED;
    }
    *run = *p;
    run->B = n_seq;
    run->N = max_seqlen;
    run->cu = cu;
    run->n_total = p->N;
    run->Nk = 0;
    return SFA_OK;
}

int sfa_fwd_varlen(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o, float* lse,
                   const float* s_aux, const int32_t* cu_seqlens, int n_seq, int max_seqlen, int num_sink, int window,
                   float scale, unsigned flags, void* stream) {
    g_err[0] = 0;
    (void)flags;
    Problem p, run;
    int st = check_varlen(q, k, v, cu_seqlens, n_seq, max_seqlen, num_sink, window, scale, &p, &run);
    if (st) return st;
    if ((st = check_tensor(o, "o")) || (st = same_shape(q, o, "q", "o"))) return st;
    if (p.Hq == 0 || p.N == 0) return SFA_OK;
    SFA_CHECK_ARG(lse != nullptr, "lse: null pointer");
    return fwd_mfma(q, k, v, o, lse, s_aux, run, (hipStream_t)stream);
}

int sfa_bwd_varlen(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o,
                   const sfa_tensor* d_o, const float* lse, const float* s_aux, const sfa_tensor* dq,
                   const sfa_tensor* dk, const sfa_tensor* dv, float* ds_aux, const int32_t* cu_seqlens, int n_seq,
                   int max_seqlen, void* workspace, size_t workspace_bytes, int num_sink, int window, float scale,
                   unsigned flags, void* stream) {
    g_err[0] = 0;
    (void)flags;
    Problem p, run;
    int st = check_varlen(q, k, v, cu_seqlens, n_seq, max_seqlen, num_sink, window, scale, &p, &run);
    if (st) return st;
    if ((st = check_tensor(o, "o")) || (st = same_shape(q, o, "q", "o"))) return st;
    if ((st = check_tensor(d_o, "do")) || (st = same_shape(q, d_o, "q", "do"))) return st;
    if ((st = check_tensor(dq, "dq")) || (st = same_shape(q, dq, "q", "dq"))) return st;
    if ((st = check_tensor(dk, "dk")) || (st = same_shape(k, dk, "k", "dk"))) return st;
    if ((st = check_tensor(dv, "dv")) || (st = same_shape(v, dv, "v", "dv"))) return st;
    if (p.Hq == 0 || p.N == 0) return SFA_OK;
    SFA_CHECK_ARG(lse != nullptr, "lse: null pointer");
    SFA_CHECK_ARG((s_aux == nullptr) == (ds_aux == nullptr), "ds_aux must be given iff s_aux is");
    if ((st = bwd_mfma_refused(q, k, v, d_o, dq, dk, dv, run))) return st;                // before the preprocess: nothing written
    const BwdWorkspace w = bwd_layout(p, q->dtype, true, 0);      // same carving as sfa_bwd with B = 1, N = total rows
    if (workspace == nullptr || workspace_bytes < w.total || ((uintptr_t)workspace & 255) != 0) {
        set_error("bwd workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", w.total, workspace_bytes,
                  workspace);
        return SFA_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    float* delta = reinterpret_cast<float*>((char*)workspace + w.delta_off);
    float* dsaux_part = reinterpret_cast<float*>((char*)workspace + w.dsaux_off);
    record_stage(0, s);
    const bool fuse = bwd_mfma_wants_consts() && bwd_preprocess_vectorised(o, d_o, p);
    st = bwd_preprocess(o, d_o, lse, s_aux, delta, dsaux_part, ds_aux, p, s,           // row-wise: no sequence structure
                        fuse ? reinterpret_cast<float*>((char*)workspace + w.mfma_off) : nullptr,
                        bwd_mfma_lse_factor(run, flags));   // (the LAUNCH problem: the kernel choice clamps the window to max_seqlen)
    record_stage(1, s);
    if (st) return st;
    st = bwd_mfma(q, k, v, d_o, lse, delta, dq, dk, dv, (char*)workspace + w.mfma_off, run, flags, s, fuse);
    record_stage(3, s);
    return st;
}

size_t sfa_decode_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t Nkv, int64_t D, int dtype) {
    DecodePlan pl;
    if (decode_plan(B, Hq, Hkv, Nkv, D, dtype, &pl) != SFA_OK) return 0;
    // int32 counters [B * Hkv + 1] of the one-pass mode (fixed place: the start), then the split partials.  Sized for
    // pl.max_splits, the largest split count ANY key count <= Nkv can plan (the split count itself is not monotonic
    // in Nkv once the workgroup target caps it), so a workspace sized for a ring's capacity serves every fill level.
    return decode_counter_bytes(B, Hkv) + align256((size_t)B * Hq * pl.max_splits * (size_t)(D + 2) * sizeof(float));
}

}  // extern "C"

namespace {

// shared by sfa_decode (one contiguous key segment) and sfa_decode_ring (sink buffer + window ring)
int decode_common(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, int64_t n1, const sfa_tensor* k2,
                  const sfa_tensor* v2, int64_t n2, const sfa_tensor* o, const float* s_aux, void* workspace,
                  size_t workspace_bytes, float scale, void* stream, const sfa_tensor* k_new = nullptr,
                  const sfa_tensor* v_new = nullptr, int64_t new_slot = -1, int* dyn_state = nullptr,
                  unsigned flags = 0, bool state_rows = false, const int32_t* slots = nullptr, bool pool = false) {
    g_err[0] = 0;
    int st;
    if ((st = check_tensor(q, "q")) || (st = check_tensor(k, "k")) || (st = check_tensor(v, "v")) ||
        (st = check_tensor(o, "o")))
        return st;
    if ((st = same_shape(k, v, "k", "v")) || (st = same_shape(q, o, "q", "o"))) return st;
    SFA_CHECK_ARG(q->dtype == k->dtype, "q and k differ in dtype");
    // decode_kernel.py:146-147
    SFA_CHECK_ARG(q->shape[2] == 1, "sink_decode_attention requires N_q=1, got %lld", (long long)q->shape[2]);
    // pool (sfa_decode_ring_step_slots): the cache buffers hold S >= 1 slots, q / k_new / v_new / o the B batch rows
    if (pool)
        SFA_CHECK_ARG(k->shape[0] >= 1 && k->shape[0] < (1ll << 30),
                      "pool: the cache buffers need shape[0] = S slots, 1 <= S < 2^30 (got %lld)", (long long)k->shape[0]);
    SFA_CHECK_ARG((pool || q->shape[0] == k->shape[0]) && q->shape[3] == k->shape[3], "q/k batch or head-dim mismatch");
    SFA_CHECK_ARG(k->shape[1] > 0 && q->shape[1] % k->shape[1] == 0, "H_q (%lld) must be divisible by H_kv (%lld)",
                  (long long)q->shape[1], (long long)k->shape[1]);
    SFA_CHECK_ARG(std::isfinite(scale), "scale must be finite");
    SFA_CHECK_ARG(n1 >= 0 && n1 <= k->shape[2], "first key segment: %lld valid rows of %lld", (long long)n1,
                  (long long)k->shape[2]);
    if (k2 || v2 || n2) {
        SFA_CHECK_ARG(k2 && v2, "second key segment needs both k and v");
        if ((st = check_tensor(k2, "k2")) || (st = check_tensor(v2, "v2")) || (st = same_shape(k2, v2, "k2", "v2")))
            return st;
        if (pool)
            SFA_CHECK_ARG(k2->shape[0] == k->shape[0], "pool: sink and window buffers must share shape[0] = S (sink %lld, window %lld)",
                          (long long)k->shape[0], (long long)k2->shape[0]);
        SFA_CHECK_ARG(k2->dtype == k->dtype && k2->shape[0] == k->shape[0] && k2->shape[1] == k->shape[1] &&
                          k2->shape[3] == k->shape[3],
                      "the two key segments must agree in dtype, batch, heads and head dim");
        SFA_CHECK_ARG(n2 >= 0 && n2 <= k2->shape[2], "second key segment: %lld valid rows of %lld", (long long)n2,
                      (long long)k2->shape[2]);
    }
    SFA_CHECK_ARG(n1 + n2 < (1ll << 31) - 4096, "N_kv too large");
    if (k_new || v_new) {       // fused cache step: the new token's K/V, stored into ring slot new_slot by the kernel
        SFA_CHECK_ARG(k_new && v_new && k2 && v2, "fused step needs k_new, v_new and the window ring");
        if ((st = check_tensor(k_new, "k_new")) || (st = check_tensor(v_new, "v_new")) ||
            (st = same_shape(k_new, v_new, "k_new", "v_new")))
            return st;
        if (pool)
            SFA_CHECK_ARG(k_new->shape[0] == q->shape[0], "q, k_new, v_new and o must share shape[0] = B (q %lld, k_new %lld)",
                          (long long)q->shape[0], (long long)k_new->shape[0]);
        SFA_CHECK_ARG(k_new->dtype == k2->dtype && (pool || k_new->shape[0] == k2->shape[0]) && k_new->shape[1] == k2->shape[1] &&
                          k_new->shape[2] == 1 && k_new->shape[3] == k2->shape[3],
                      "k_new / v_new must be [B, H_kv, 1, D] in the ring's dtype");
        SFA_CHECK_ARG(dyn_state || (new_slot >= 0 && new_slot < n2), "write slot %lld outside the %lld valid ring slots",
                      (long long)new_slot, (long long)n2);
    }
    if (q->shape[0] == 0 || q->shape[1] == 0) return SFA_OK;
    DecodePlan pl;
    st = decode_plan(q->shape[0], q->shape[1], k->shape[1], n1 + n2, q->shape[3], q->dtype, &pl);
    if (st) return st;
    const int es = dtype_size(q->dtype);
    const sfa_tensor* ts[7] = {q, k, v, k2, v2, k_new, v_new};
    for (const sfa_tensor* t : ts) {
        if (!t || t->shape[2] == 0) continue;
        SFA_CHECK_ARG(((uintptr_t)t->ptr % 16) == 0 && (t->stride[0] * es) % 16 == 0 && (t->stride[1] * es) % 16 == 0 &&
                          (t->stride[2] * es) % 16 == 0,
                      "decode: q/k/v rows must be 16-byte aligned");
    }
    const size_t need = sfa_decode_workspace_bytes(q->shape[0], q->shape[1], k->shape[1], n1 + n2, q->shape[3], q->dtype);
    if (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace & 255) != 0) {
        set_error("decode workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", need, workspace_bytes,
                  workspace);
        return SFA_ERR_WORKSPACE;
    }
    return decode_launch(q, k, v, n1, n2 ? k2 : nullptr, n2 ? v2 : nullptr, n2, o, s_aux, workspace, scale, pl,
                         (hipStream_t)stream, k_new, v_new, (int)new_slot, dyn_state,
                         (flags & SFA_FLAG_DECODE_ONE_PASS) != 0, state_rows, slots);
}

}  // namespace

extern "C" {

int sfa_decode(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o,
               const float* s_aux, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
               void* stream) {
    return decode_common(q, k, v, k ? k->shape[2] : 0, nullptr, nullptr, 0, o, s_aux, workspace, workspace_bytes, scale,
                         stream, nullptr, nullptr, -1, nullptr, flags);
}

int sfa_decode_ring(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                    const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len, const sfa_tensor* o,
                    const float* s_aux, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                    void* stream) {
    return decode_common(q, sink_k, sink_v, sink_len, window_k, window_v, window_len, o, s_aux, workspace,
                         workspace_bytes, scale, stream, nullptr, nullptr, -1, nullptr, flags);
}

int sfa_decode_ring_step(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                         const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                         int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                         const float* s_aux, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                         void* stream) {
    g_err[0] = 0;
    SFA_CHECK_ARG(k_new != nullptr && v_new != nullptr, "k_new / v_new: null tensor descriptor");
    return decode_common(q, sink_k, sink_v, sink_len, window_k, window_v, window_len, o, s_aux, workspace,
                         workspace_bytes, scale, stream, k_new, v_new, write_pos, nullptr, flags);
}

int sfa_decode_ring_step_dyn(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                             const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                             const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int32_t* state,
                             void* workspace, size_t workspace_bytes, float scale, unsigned flags, void* stream) {
    g_err[0] = 0;
    SFA_CHECK_ARG(k_new != nullptr && v_new != nullptr, "k_new / v_new: null tensor descriptor");
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(sink_k != nullptr && window_k != nullptr, "cache buffers: null tensor descriptor");
    // launch geometry and workspace are sized for the FULL cache (every sink row, every ring slot)
    return decode_common(q, sink_k, sink_v, sink_k->shape[2], window_k, window_v, window_k->shape[2], o, s_aux,
                         workspace, workspace_bytes, scale, stream, k_new, v_new, 0, state, flags);
}

int sfa_decode_ring_step_rows(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                              const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                              const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int32_t* state,
                              void* workspace, size_t workspace_bytes, float scale, unsigned flags, void* stream) {
    g_err[0] = 0;
    SFA_CHECK_ARG(k_new != nullptr && v_new != nullptr, "k_new / v_new: null tensor descriptor");
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(sink_k != nullptr && window_k != nullptr, "cache buffers: null tensor descriptor");
    // the state rows [B][4] are per batch row of the cache buffers (decode_common checks q / k_new against them)
    return decode_common(q, sink_k, sink_v, sink_k->shape[2], window_k, window_v, window_k->shape[2], o, s_aux,
                         workspace, workspace_bytes, scale, stream, k_new, v_new, 0, state, flags, true);
}

int sfa_decode_ring_step_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                               const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                               const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int32_t* state,
                               const int32_t* slots, void* workspace, size_t workspace_bytes, float scale,
                               unsigned flags, void* stream) {
    g_err[0] = 0;
    SFA_CHECK_ARG(k_new != nullptr && v_new != nullptr, "k_new / v_new: null tensor descriptor");
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(slots != nullptr, "slots: null device pointer");
    SFA_CHECK_ARG(sink_k != nullptr && window_k != nullptr, "cache buffers: null tensor descriptor");
    // plan, grid and workspace are those of the rows call for q's B rows at the full cache; the buffers are the pool
    return decode_common(q, sink_k, sink_v, sink_k->shape[2], window_k, window_v, window_k->shape[2], o, s_aux,
                         workspace, workspace_bytes, scale, stream, k_new, v_new, 0, state, flags, true, slots, true);
}

}  // extern "C"

namespace {

// every host-checkable argument of sfa_decode_ring_multi(_dyn); nothing launches
int check_multi(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len, int64_t write_pos,
                const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o, float scale, bool pool = false) {
    int st;
    if ((st = check_tensor(q, "q")) || (st = check_tensor(o, "o")) || (st = check_tensor(sink_k, "sink_k")) ||
        (st = check_tensor(sink_v, "sink_v")) || (st = check_tensor(window_k, "window_k")) ||
        (st = check_tensor(window_v, "window_v")) || (st = check_tensor(k_new, "k_new")) ||
        (st = check_tensor(v_new, "v_new")))
        return st;
    if ((st = same_shape(q, o, "q", "o")) || (st = same_shape(sink_k, sink_v, "sink_k", "sink_v")) ||
        (st = same_shape(window_k, window_v, "window_k", "window_v")) || (st = same_shape(k_new, v_new, "k_new", "v_new")))
        return st;
    const int64_t B = q->shape[0], Hq = q->shape[1], n = q->shape[2], D = q->shape[3], Hkv = k_new->shape[1];
    const int64_t Wc = window_k->shape[2];
    SFA_CHECK_ARG(q->dtype == sink_k->dtype && q->dtype == window_k->dtype && q->dtype == k_new->dtype,
                  "q, the cache buffers and k_new / v_new must share one dtype");
    SFA_CHECK_ARG(n >= 1, "decode_multi: the chunk needs at least one token");
    SFA_CHECK_ARG(k_new->shape[0] == B && k_new->shape[2] == n && k_new->shape[3] == D,
                  "k_new / v_new must be [B, H_kv, n, D] with the n = %lld rows of q", (long long)n);
    SFA_CHECK_ARG(Hkv > 0 && Hq % Hkv == 0, "H_q (%lld) must be divisible by H_kv (%lld)", (long long)Hq, (long long)Hkv);
    if (pool) {     // *_slots: the buffers hold S >= 1 slots, the activations B batch rows
        SFA_CHECK_ARG(sink_k->shape[0] >= 1 && sink_k->shape[0] == window_k->shape[0],
                      "pool: sink and window buffers must share shape[0] = S >= 1 (sink %lld, window %lld)",
                      (long long)sink_k->shape[0], (long long)window_k->shape[0]);
        SFA_CHECK_ARG(sink_k->shape[0] < (1ll << 30), "problem too large");
    }
    SFA_CHECK_ARG((pool || sink_k->shape[0] == B) && sink_k->shape[1] == Hkv && sink_k->shape[3] == D &&
                      (pool || window_k->shape[0] == B) && window_k->shape[1] == Hkv && window_k->shape[3] == D,
                  "sink / window buffers must be [B, H_kv, *, D] like k_new");
    SFA_CHECK_ARG(Wc >= 1, "the ring needs a capacity of at least one slot");
    SFA_CHECK_ARG(sink_len >= 0 && sink_len <= sink_k->shape[2], "sink_len %lld outside [0, %lld]", (long long)sink_len,
                  (long long)sink_k->shape[2]);
    SFA_CHECK_ARG(window_len >= 0 && window_len <= Wc, "window_len %lld outside [0, %lld]", (long long)window_len,
                  (long long)Wc);
    SFA_CHECK_ARG(write_pos >= 0 && write_pos < Wc, "write_pos %lld outside [0, %lld)", (long long)write_pos, (long long)Wc);
    SFA_CHECK_ARG(window_len == Wc || write_pos == window_len,
                  "write_pos (%lld) must equal window_len (%lld) until the ring is full", (long long)write_pos,
                  (long long)window_len);
    SFA_CHECK_ARG(std::isfinite(scale), "scale must be finite");
    SFA_CHECK_ARG(sink_len + window_len + n < (1ll << 30) && B * Hq * n < (1ll << 30) && Wc < (1ll << 30),
                  "problem too large");
    if ((st = decode_multi_check_head_dim(D, q->dtype))) return st;
    const int es = dtype_size(q->dtype);
    const sfa_tensor* ts[8] = {q, o, sink_k, sink_v, window_k, window_v, k_new, v_new};
    for (const sfa_tensor* t : ts) {
        if (t->shape[0] == 0 || t->shape[1] == 0 || t->shape[2] == 0) continue;
        SFA_CHECK_ARG(((uintptr_t)t->ptr % 16) == 0 && (t->stride[0] * es) % 16 == 0 && (t->stride[1] * es) % 16 == 0 &&
                          (t->stride[2] * es) % 16 == 0,
                      "decode_multi: rows of every tensor must be 16-byte aligned");
    }
    return SFA_OK;
}

int check_multi_workspace(const sfa_tensor* q, const sfa_tensor* k_new, int64_t Nkv, void* workspace,
                          size_t workspace_bytes) {
    const size_t need = decode_multi_workspace(q->shape[0], q->shape[1], k_new->shape[1], q->shape[2], Nkv, q->shape[3],
                                               q->dtype);
    if (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace & 255) != 0) {
        set_error("decode_multi workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", need, workspace_bytes,
                  workspace);
        return SFA_ERR_WORKSPACE;
    }
    return SFA_OK;
}

}  // namespace

extern "C" {

size_t sfa_decode_multi_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t n_new, int64_t Nkv, int64_t D,
                                        int dtype) {
    return decode_multi_workspace(B, Hq, Hkv, n_new, Nkv, D, dtype);
}

int sfa_decode_ring_multi(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                          const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                          int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                          const float* s_aux, int commit, void* workspace, size_t workspace_bytes, float scale,
                          unsigned flags, void* stream) {
    g_err[0] = 0;
    int st;
    if ((st = check_multi(q, sink_k, sink_v, sink_len, window_k, window_v, window_len, write_pos, k_new, v_new, o, scale)))
        return st;
    if (q->shape[0] == 0 || q->shape[1] == 0) return SFA_OK;
    if ((st = check_multi_workspace(q, k_new, sink_len + window_len + q->shape[2], workspace, workspace_bytes))) return st;
    return decode_multi_launch(q, sink_k, sink_v, sink_len, window_k, window_v, window_len, write_pos, k_new, v_new, o,
                               s_aux, commit, workspace, scale, flags, (hipStream_t)stream);
}

int sfa_decode_ring_multi_dyn(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                              const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                              const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit,
                              int32_t* state, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                              void* stream) {
    g_err[0] = 0;
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(sink_k != nullptr && window_k != nullptr, "cache buffers: null tensor descriptor");
    // every check of the host-state call, at the full cache (the launch geometry and workspace cover every fill level)
    const int64_t ns = sink_k->shape[2], Wc = window_k->shape[2];
    int st;
    if ((st = check_multi(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, scale))) return st;
    if (q->shape[0] == 0 || q->shape[1] == 0) {
        if (!commit) return SFA_OK;
        return ring_commit_dyn_launch(window_k, window_v, k_new, v_new, nullptr, state, (hipStream_t)stream);
    }
    if ((st = check_multi_workspace(q, k_new, ns + Wc + q->shape[2], workspace, workspace_bytes))) return st;
    return decode_multi_launch(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, s_aux, commit, workspace,
                               scale, flags, (hipStream_t)stream, state);
}

int sfa_decode_ring_multi_rows(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                               const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                               const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit,
                               int32_t* state, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                               void* stream) {
    g_err[0] = 0;
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(sink_k != nullptr && window_k != nullptr, "cache buffers: null tensor descriptor");
    const int64_t ns = sink_k->shape[2], Wc = window_k->shape[2];
    int st;
    if ((st = check_multi(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, scale))) return st;
    if (q->shape[0] == 0) return SFA_OK;               // no rows: no state to read or advance
    if (q->shape[1] == 0) {
        if (!commit) return SFA_OK;
        return ring_commit_dyn_launch(window_k, window_v, k_new, v_new, nullptr, state, (hipStream_t)stream, true);
    }
    if ((st = check_multi_workspace(q, k_new, ns + Wc + q->shape[2], workspace, workspace_bytes))) return st;
    return decode_multi_launch(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, s_aux, commit, workspace,
                               scale, flags, (hipStream_t)stream, state, true);
}

int sfa_decode_ring_multi_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                                const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit,
                                int32_t* state, const int32_t* slots, void* workspace, size_t workspace_bytes,
                                float scale, unsigned flags, void* stream) {
    g_err[0] = 0;
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(slots != nullptr, "slots: null device pointer");
    SFA_CHECK_ARG(sink_k != nullptr && window_k != nullptr, "cache buffers: null tensor descriptor");
    const int64_t ns = sink_k->shape[2], Wc = window_k->shape[2];
    int st;
    if ((st = check_multi(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, scale, true))) return st;
    if (q->shape[0] == 0) return SFA_OK;               // no rows: no state to read or advance
    if (q->shape[1] == 0) {
        if (!commit) return SFA_OK;
        return ring_commit_dyn_launch(window_k, window_v, k_new, v_new, nullptr, state, (hipStream_t)stream, true, nullptr,
                                      0, slots);
    }
    if ((st = check_multi_workspace(q, k_new, ns + Wc + q->shape[2], workspace, workspace_bytes))) return st;
    return decode_multi_launch(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, s_aux, commit, workspace,
                               scale, flags, (hipStream_t)stream, state, true, nullptr, 0, slots);
}

size_t sfa_decode_ragged_workspace_bytes(int64_t n_seq, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache,
                                         int64_t D, int dtype) {
    return decode_ragged_workspace(n_seq, Hq, Hkv, T, Nkv_cache, D, dtype);
}

int sfa_decode_ring_ragged_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                 const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                                 const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit,
                                 int32_t* state, const int32_t* slots, const int32_t* cu_q, int n_seq,
                                 void* workspace, size_t workspace_bytes, float scale, unsigned flags, void* stream) {
    g_err[0] = 0;
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(slots != nullptr, "slots: null device pointer");
    SFA_CHECK_ARG(cu_q != nullptr, "cu_q: null device pointer");
    SFA_CHECK_ARG(n_seq >= 1, "decode_ragged: n_seq (%d) must be at least 1", n_seq);
    SFA_CHECK_ARG(sink_k != nullptr && window_k != nullptr, "cache buffers: null tensor descriptor");
    const int64_t ns = sink_k->shape[2], Wc = window_k->shape[2];
    int st;
    // every check of the slots call at the full cache; q / k_new / v_new / o share shape[0] and T there
    if ((st = check_multi(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, scale, true))) return st;
    SFA_CHECK_ARG(q->shape[0] == 1, "decode_ragged: q / k_new / v_new / o must be packed [1, H, T, D] (got shape[0] = %lld)",
                  (long long)q->shape[0]);
    SFA_CHECK_ARG(q->shape[1] >= 1, "decode_ragged: H_q must be at least 1");
    const size_t need = decode_ragged_workspace(n_seq, q->shape[1], k_new->shape[1], q->shape[2], ns + Wc, q->shape[3],
                                                q->dtype);
    if (need == 0 || workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace & 255) != 0) {
        set_error("decode_ragged workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", need, workspace_bytes,
                  workspace);
        return SFA_ERR_WORKSPACE;
    }
    return decode_ragged_launch(q, sink_k, sink_v, window_k, window_v, k_new, v_new, o, s_aux, commit, state, slots, cu_q,
                                n_seq, workspace, scale, flags, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// the tree-specific checks of sfa_decode_ring_tree*, after check_multi
int check_tree(const sfa_tensor* q, const int32_t* parent, int64_t parent_bstride) {
    const int64_t n = q->shape[2];
    SFA_CHECK_ARG(n <= 64, "decode_tree: a tree chunk holds at most 64 nodes (got n = %lld)", (long long)n);
    SFA_CHECK_ARG(parent != nullptr, "parent: null device pointer");
    SFA_CHECK_ARG(parent_bstride == 0 || (parent_bstride >= n && parent_bstride < (1ll << 30)),
                  "parent_bstride %lld: 0 (one tree shared by the batch) or >= n = %lld (one row per sequence)",
                  (long long)parent_bstride, (long long)n);
    return SFA_OK;
}

}  // namespace

extern "C" {

int sfa_decode_ring_tree(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                         const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                         int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                         const float* s_aux, const int32_t* parent, int64_t parent_bstride, void* workspace,
                         size_t workspace_bytes, float scale, unsigned flags, void* stream) {
    g_err[0] = 0;
    int st;
    if ((st = check_multi(q, sink_k, sink_v, sink_len, window_k, window_v, window_len, write_pos, k_new, v_new, o, scale)))
        return st;
    if ((st = check_tree(q, parent, parent_bstride))) return st;
    if (q->shape[0] == 0 || q->shape[1] == 0) return SFA_OK;
    if ((st = check_multi_workspace(q, k_new, sink_len + window_len + q->shape[2], workspace, workspace_bytes))) return st;
    return decode_multi_launch(q, sink_k, sink_v, sink_len, window_k, window_v, window_len, write_pos, k_new, v_new, o,
                               s_aux, 0, workspace, scale, flags, (hipStream_t)stream, nullptr, false, parent,
                               parent_bstride);
}

static int tree_dyn(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                    const sfa_tensor* window_v, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                    const float* s_aux, const int32_t* parent, int64_t parent_bstride, int32_t* state, void* workspace,
                    size_t workspace_bytes, float scale, unsigned flags, void* stream, bool rows,
                    const int32_t* slots = nullptr, bool pool = false) {
    g_err[0] = 0;
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(!pool || slots != nullptr, "slots: null device pointer");
    SFA_CHECK_ARG(sink_k != nullptr && window_k != nullptr, "cache buffers: null tensor descriptor");
    const int64_t ns = sink_k->shape[2], Wc = window_k->shape[2];
    int st;
    if ((st = check_multi(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, scale, pool))) return st;
    if ((st = check_tree(q, parent, parent_bstride))) return st;
    if (q->shape[0] == 0 || q->shape[1] == 0) return SFA_OK;   // nothing to attend; a tree call never commits
    if ((st = check_multi_workspace(q, k_new, ns + Wc + q->shape[2], workspace, workspace_bytes))) return st;
    return decode_multi_launch(q, sink_k, sink_v, ns, window_k, window_v, Wc, 0, k_new, v_new, o, s_aux, 0, workspace,
                               scale, flags, (hipStream_t)stream, state, rows, parent, parent_bstride, slots);
}

int sfa_decode_ring_tree_dyn(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                             const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                             const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, const int32_t* parent,
                             int64_t parent_bstride, int32_t* state, void* workspace, size_t workspace_bytes,
                             float scale, unsigned flags, void* stream) {
    return tree_dyn(q, sink_k, sink_v, window_k, window_v, k_new, v_new, o, s_aux, parent, parent_bstride, state,
                    workspace, workspace_bytes, scale, flags, stream, false);
}

int sfa_decode_ring_tree_rows(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                              const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                              const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, const int32_t* parent,
                              int64_t parent_bstride, int32_t* state, void* workspace, size_t workspace_bytes,
                              float scale, unsigned flags, void* stream) {
    return tree_dyn(q, sink_k, sink_v, window_k, window_v, k_new, v_new, o, s_aux, parent, parent_bstride, state,
                    workspace, workspace_bytes, scale, flags, stream, true);
}

int sfa_decode_ring_tree_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                               const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                               const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, const int32_t* parent,
                               int64_t parent_bstride, int32_t* state, const int32_t* slots, void* workspace,
                               size_t workspace_bytes, float scale, unsigned flags, void* stream) {
    return tree_dyn(q, sink_k, sink_v, window_k, window_v, k_new, v_new, o, s_aux, parent, parent_bstride, state,
                    workspace, workspace_bytes, scale, flags, stream, true, slots, true);
}

}  // extern "C"

namespace {

// every host-checkable argument of sfa_ring_commit_dyn / _rows; nothing launches
int check_commit(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                 const sfa_tensor* v_new, const int32_t* count, int32_t* state, bool pool = false) {
    int st;
    if ((st = check_tensor(window_k, "window_k")) || (st = check_tensor(window_v, "window_v")) ||
        (st = check_tensor(k_new, "k_new")) || (st = check_tensor(v_new, "v_new")))
        return st;
    if ((st = same_shape(window_k, window_v, "window_k", "window_v")) || (st = same_shape(k_new, v_new, "k_new", "v_new")))
        return st;
    SFA_CHECK_ARG(count != nullptr, "count: null device pointer");
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(k_new->dtype == window_k->dtype, "k_new / v_new and the ring must share one dtype");
    const int64_t n = k_new->shape[2], Wc = window_k->shape[2];
    SFA_CHECK_ARG(n >= 1, "ring_commit: the chunk needs at least one token");
    SFA_CHECK_ARG(Wc >= 1, "the ring needs a capacity of at least one slot");
    if (pool)
        SFA_CHECK_ARG(window_k->shape[0] >= 1 && window_k->shape[0] < (1ll << 30),
                      "pool: the ring needs shape[0] = S >= 1 slots (got %lld)", (long long)window_k->shape[0]);
    SFA_CHECK_ARG((pool || k_new->shape[0] == window_k->shape[0]) && k_new->shape[1] == window_k->shape[1] &&
                      k_new->shape[3] == window_k->shape[3],
                  "k_new / v_new must be [B, H_kv, n, D] like the ring [B, H_kv, Wc, D]");
    SFA_CHECK_ARG(n < (1ll << 30) && Wc < (1ll << 30), "problem too large");
    const int es = dtype_size(k_new->dtype);
    SFA_CHECK_ARG(k_new->shape[3] > 0 && (k_new->shape[3] * es) % 16 == 0,
                  "ring_commit: K/V rows must be a multiple of 16 bytes (head dim %lld)", (long long)k_new->shape[3]);
    const sfa_tensor* ts[4] = {window_k, window_v, k_new, v_new};
    for (const sfa_tensor* t : ts) {
        if (t->shape[0] == 0 || t->shape[1] == 0) continue;
        SFA_CHECK_ARG(((uintptr_t)t->ptr % 16) == 0 && (t->stride[0] * es) % 16 == 0 && (t->stride[1] * es) % 16 == 0 &&
                          (t->stride[2] * es) % 16 == 0,
                      "ring_commit: rows of every tensor must be 16-byte aligned");
    }
    return SFA_OK;
}

}  // namespace

extern "C" {

int sfa_ring_commit_dyn(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                        const sfa_tensor* v_new, const int32_t* count, int32_t* state, void* stream) {
    g_err[0] = 0;
    int st;
    if ((st = check_commit(window_k, window_v, k_new, v_new, count, state))) return st;
    return ring_commit_dyn_launch(window_k, window_v, k_new, v_new, count, state, (hipStream_t)stream);
}

int sfa_ring_commit_rows(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                         const sfa_tensor* v_new, const int32_t* count, int32_t* state, void* stream) {
    g_err[0] = 0;
    int st;
    if ((st = check_commit(window_k, window_v, k_new, v_new, count, state))) return st;
    if (k_new->shape[0] == 0) return SFA_OK;
    return ring_commit_dyn_launch(window_k, window_v, k_new, v_new, count, state, (hipStream_t)stream, true);
}

static int commit_path(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                       const sfa_tensor* v_new, const int32_t* count, const int32_t* path, int64_t path_bstride,
                       int32_t* state, void* stream, bool rows, const int32_t* slots = nullptr, bool pool = false) {
    g_err[0] = 0;
    int st;
    SFA_CHECK_ARG(!pool || slots != nullptr, "slots: null device pointer");
    if ((st = check_commit(window_k, window_v, k_new, v_new, count, state, pool))) return st;
    const int64_t n = k_new->shape[2];
    SFA_CHECK_ARG(path != nullptr, "path: null device pointer");
    SFA_CHECK_ARG(path_bstride == 0 || (path_bstride >= n && path_bstride < (1ll << 30)),
                  "path_bstride %lld: 0 (one path shared by the batch) or >= n = %lld (one row per sequence)",
                  (long long)path_bstride, (long long)n);
    if (rows && k_new->shape[0] == 0) return SFA_OK;
    return ring_commit_dyn_launch(window_k, window_v, k_new, v_new, count, state, (hipStream_t)stream, rows, path,
                                  path_bstride, slots);
}

int sfa_ring_commit_path_dyn(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                             const sfa_tensor* v_new, const int32_t* count, const int32_t* path, int64_t path_bstride,
                             int32_t* state, void* stream) {
    return commit_path(window_k, window_v, k_new, v_new, count, path, path_bstride, state, stream, false);
}

int sfa_ring_commit_path_rows(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                              const sfa_tensor* v_new, const int32_t* count, const int32_t* path, int64_t path_bstride,
                              int32_t* state, void* stream) {
    return commit_path(window_k, window_v, k_new, v_new, count, path, path_bstride, state, stream, true);
}

int sfa_ring_commit_slots(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                          const sfa_tensor* v_new, const int32_t* count, int32_t* state, const int32_t* slots,
                          void* stream) {
    g_err[0] = 0;
    int st;
    SFA_CHECK_ARG(slots != nullptr, "slots: null device pointer");
    if ((st = check_commit(window_k, window_v, k_new, v_new, count, state, true))) return st;
    if (k_new->shape[0] == 0) return SFA_OK;
    return ring_commit_dyn_launch(window_k, window_v, k_new, v_new, count, state, (hipStream_t)stream, true, nullptr, 0,
                                  slots);
}

int sfa_ring_commit_path_slots(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                               const sfa_tensor* v_new, const int32_t* count, const int32_t* path, int64_t path_bstride,
                               int32_t* state, const int32_t* slots, void* stream) {
    return commit_path(window_k, window_v, k_new, v_new, count, path, path_bstride, state, stream, true, slots, true);
}

}  // extern "C"

namespace {

// sfa_ring_fill_varlen (slots null: sequence i -> cache row i of n_seq) and sfa_ring_fill_varlen_slots (pool)
int fill_varlen(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v, const int32_t* cu_seqlens,
                int n_seq, int32_t* state, void* stream, const int32_t* slots, bool pool) {
    g_err[0] = 0;
    int st;
    if ((st = check_tensor(sink_k, "sink_k")) || (st = check_tensor(sink_v, "sink_v")) ||
        (st = check_tensor(window_k, "window_k")) || (st = check_tensor(window_v, "window_v")) ||
        (st = check_tensor(k, "k")) || (st = check_tensor(v, "v")))
        return st;
    if ((st = same_shape(sink_k, sink_v, "sink_k", "sink_v")) ||
        (st = same_shape(window_k, window_v, "window_k", "window_v")) || (st = same_shape(k, v, "k", "v")))
        return st;
    SFA_CHECK_ARG(cu_seqlens != nullptr, "cu_seqlens: null device pointer");
    SFA_CHECK_ARG(state != nullptr, "state: null device pointer");
    SFA_CHECK_ARG(!pool || slots != nullptr, "slots: null device pointer");
    SFA_CHECK_ARG(n_seq >= 1, "n_seq must be >= 1 (got %d)", n_seq);
    SFA_CHECK_ARG(k->shape[0] == 1, "packed layout: k / v must be [1, H_kv, T, D] (batch dim %lld)", (long long)k->shape[0]);
    SFA_CHECK_ARG(k->dtype == sink_k->dtype && k->dtype == window_k->dtype,
                  "k / v and the cache buffers must share one dtype");
    const int64_t Hkv = k->shape[1], D = k->shape[3], Wc = window_k->shape[2];
    if (pool)
        SFA_CHECK_ARG(sink_k->shape[0] >= 1 && sink_k->shape[0] == window_k->shape[0] && sink_k->shape[0] < (1ll << 30),
                      "pool: sink and window buffers must share shape[0] = S >= 1 (sink %lld, window %lld)",
                      (long long)sink_k->shape[0], (long long)window_k->shape[0]);
    else
        SFA_CHECK_ARG(sink_k->shape[0] == n_seq && window_k->shape[0] == n_seq,
                      "n_seq (%d) must match the cache buffers' batch (sink %lld, window %lld)", n_seq,
                      (long long)sink_k->shape[0], (long long)window_k->shape[0]);
    SFA_CHECK_ARG(sink_k->shape[1] == Hkv && sink_k->shape[3] == D && window_k->shape[1] == Hkv && window_k->shape[3] == D,
                  "sink / window buffers must be [n_seq, H_kv, *, D] like k");
    SFA_CHECK_ARG(Wc >= 1, "the ring needs a capacity of at least one slot");
    SFA_CHECK_ARG(k->shape[2] < (1ll << 30) && sink_k->shape[2] + Wc < (1ll << 30), "problem too large");
    const int es = dtype_size(k->dtype);
    SFA_CHECK_ARG(D > 0 && (D * es) % 16 == 0, "ring_fill_varlen: K/V rows must be a multiple of 16 bytes (head dim %lld)",
                  (long long)D);
    const sfa_tensor* ts[6] = {sink_k, sink_v, window_k, window_v, k, v};
    for (const sfa_tensor* t : ts) {
        if (t->shape[0] == 0 || t->shape[1] == 0 || t->shape[2] == 0) continue;
        SFA_CHECK_ARG(((uintptr_t)t->ptr % 16) == 0 && (t->stride[0] * es) % 16 == 0 && (t->stride[1] * es) % 16 == 0 &&
                          (t->stride[2] * es) % 16 == 0,
                      "ring_fill_varlen: rows of every tensor must be 16-byte aligned");
    }
    return ring_fill_varlen_launch(sink_k, sink_v, window_k, window_v, k, v, cu_seqlens, n_seq, state,
                                   (hipStream_t)stream, slots);
}

}  // namespace

extern "C" {

int sfa_ring_fill_varlen(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                         const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                         const int32_t* cu_seqlens, int n_seq, int32_t* state, void* stream) {
    return fill_varlen(sink_k, sink_v, window_k, window_v, k, v, cu_seqlens, n_seq, state, stream, nullptr, false);
}

int sfa_ring_fill_varlen_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                               const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                               const int32_t* cu_seqlens, int n_seq, int32_t* state, const int32_t* slots,
                               void* stream) {
    return fill_varlen(sink_k, sink_v, window_k, window_v, k, v, cu_seqlens, n_seq, state, stream, slots, true);
}

}  // extern "C"
