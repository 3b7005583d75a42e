// extern "C" entry points of libsfa.so (declared in include/sfa.h): argument
// validation, kernel-family choice, workspace carving.  No allocation, no sync.
#include <cmath>
#include <cstring>
#include <initializer_list>

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

// fp8_ok: a cache buffer of an *_fp8_slots call or of sfa_ring_copy_slots, the only places SFA_DTYPE_FP8_E4M3 is legal
int check_tensor(const sfa_tensor* t, const char* name, bool fp8_ok = false) {
    SFA_CHECK_ARG(t != nullptr, "%s: null tensor descriptor", name);
    SFA_CHECK_ARG(t->dtype == SFA_DTYPE_F32 || t->dtype == SFA_DTYPE_F16 || t->dtype == SFA_DTYPE_BF16 ||
                      (fp8_ok && t->dtype == SFA_DTYPE_FP8_E4M3),
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

// ------------------------------------------------------------------------------------------------ sink + ring cache
// Every entry point below fills a RingCall (sfa_internal.hpp) with what its signature provides and hands it to its
// family: ring_step, ring_multi / ring_tree, ring_ragged, ring_commit / ring_commit_path, fill_varlen, copy_slots (two
// pools, no RingCall).  The family
// runs the checks, the empty-shape returns, the workspace test and the launch.
namespace {

#define SFA_NEED(p, what) SFA_CHECK_ARG((p) != nullptr, what ": null device pointer")

// rows of every tensor 16-byte aligned (base and batch / head / row strides).  skip: bit i = a tensor with
// shape[i] == 0 is empty and not looked at (the rule differs between the families); a null tensor never is
int check_rows16(std::initializer_list<const sfa_tensor*> ts, int es, unsigned skip, const char* msg) {
    for (const sfa_tensor* t : ts) {
        if (!t || ((skip & 1) && t->shape[0] == 0) || ((skip & 2) && t->shape[1] == 0) || ((skip & 4) && t->shape[2] == 0))
            continue;
        SFA_CHECK_ARG(((uintptr_t)t->ptr % 16) == 0 && (t->stride[0] * es) % 16 == 0 && (t->stride[1] * es) % 16 == 0 &&
                          (t->stride[2] * es) % 16 == 0,
                      "%s", msg);
    }
    return SFA_OK;
}

// sized: `need` is a size (a workspace query that refuses the shape gives 0)
int check_workspace(const char* name, size_t need, bool sized, void* workspace, size_t workspace_bytes) {
    if (!sized || workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace & 255) != 0) {
        set_error("%s workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", name, need, workspace_bytes, workspace);
        return SFA_ERR_WORKSPACE;
    }
    return SFA_OK;
}

// the fields every attention entry point provides, in the order of its signature
RingCall attend_call(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                     const sfa_tensor* window_v, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                     const float* s_aux, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                     void* stream) {
    RingCall c{};
    c.q = q, c.sink_k = sink_k, c.sink_v = sink_v, c.window_k = window_k, c.window_v = window_v;
    c.k_new = k_new, c.v_new = v_new, c.o = o, c.s_aux = s_aux;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes;
    c.scale = scale, c.flags = flags, c.stream = (hipStream_t)stream;
    return c;
}

RingCall& host_state(RingCall& c, int64_t sink_len, int64_t window_len, int64_t write_pos) {
    c.mode = RingState::Host, c.sink_len = sink_len, c.window_len = window_len, c.write_pos = write_pos;
    return c;
}

// launch geometry and workspace are those of the FULL cache (every sink row, every ring slot)
RingCall& device_state(RingCall& c, RingState mode, int32_t* state, const int32_t* slots) {
    c.mode = mode, c.state = state, c.slots = slots;
    c.sink_len = c.sink_k ? c.sink_k->shape[2] : 0, c.window_len = c.window_k ? c.window_k->shape[2] : 0;
    return c;
}

// the null checks every device-state call shares (a *_slots entry point has checked `slots` in between)
int check_device_state(const RingCall& c) {
    if (c.mode == RingState::Host) return SFA_OK;
    SFA_NEED(c.state, "state");
    SFA_CHECK_ARG(c.sink_k != nullptr && c.window_k != nullptr, "cache buffers: null tensor descriptor");
    return SFA_OK;
}

// sfa_decode (one contiguous key segment: the "sink" buffers, no ring) and sfa_decode_ring*: one query per row.  With
// slots the cache buffers hold S >= 1 slots, q / k_new / v_new / o the B batch rows
int ring_step(const RingCall& c) {
    g_err[0] = 0;
    int st;
    if ((st = check_device_state(c))) return st;
    const sfa_tensor *q = c.q, *k = c.sink_k, *v = c.sink_v, *k2 = c.window_k, *v2 = c.window_v, *o = c.o;
    const sfa_tensor *k_new = c.k_new, *v_new = c.v_new;
    const int64_t n1 = c.sink_len, n2 = c.window_len;
    const bool pool = c.slots != nullptr;
    if ((st = check_tensor(q, "q")) || (st = check_tensor(k, "k")) || (st = check_tensor(v, "v")) ||
        (st = check_tensor(o, "o")))
        return st;
    if ((st = same_shape(k, v, "k", "v")) || (st = same_shape(q, o, "q", "o"))) return st;
    SFA_CHECK_ARG(q->dtype == k->dtype, "q and k differ in dtype");
    // decode_kernel.py:146-147
    SFA_CHECK_ARG(q->shape[2] == 1, "sink_decode_attention requires N_q=1, got %lld", (long long)q->shape[2]);
    if (pool)
        SFA_CHECK_ARG(k->shape[0] >= 1 && k->shape[0] < (1ll << 30),
                      "pool: the cache buffers need shape[0] = S slots, 1 <= S < 2^30 (got %lld)", (long long)k->shape[0]);
    SFA_CHECK_ARG((pool || q->shape[0] == k->shape[0]) && q->shape[3] == k->shape[3], "q/k batch or head-dim mismatch");
    SFA_CHECK_ARG(k->shape[1] > 0 && q->shape[1] % k->shape[1] == 0, "H_q (%lld) must be divisible by H_kv (%lld)",
                  (long long)q->shape[1], (long long)k->shape[1]);
    SFA_CHECK_ARG(std::isfinite(c.scale), "scale must be finite");
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
    if (k_new || v_new) {       // fused cache step: the new token's K/V, stored into ring slot write_pos by the kernel
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
        SFA_CHECK_ARG(c.mode != RingState::Host || (c.write_pos >= 0 && c.write_pos < n2),
                      "write slot %lld outside the %lld valid ring slots", (long long)c.write_pos, (long long)n2);
    }
    if (q->shape[0] == 0 || q->shape[1] == 0) return SFA_OK;
    DecodePlan pl;
    st = decode_plan(q->shape[0], q->shape[1], k->shape[1], n1 + n2, q->shape[3], q->dtype, &pl);
    if (st) return st;
    if ((st = check_rows16({q, k, v, k2, v2, k_new, v_new}, dtype_size(q->dtype), 4, "decode: q/k/v rows must be 16-byte aligned")))
        return st;
    const size_t need = sfa_decode_workspace_bytes(q->shape[0], q->shape[1], k->shape[1], n1 + n2, q->shape[3], q->dtype);
    if ((st = check_workspace("decode", need, true, c.workspace, c.workspace_bytes))) return st;
    return decode_launch(c, pl);
}

// The checks an *_fp8_slots call adds (`who`: its name in the messages).  Where the 16-bit call compares the dtypes: the
// cache buffers are FP8, the activations share one dtype (where it checks the head dim: check_pool_served)
int check_fp8_dtypes(const char* who, const sfa_tensor* cache_a, const sfa_tensor* cache_b, const sfa_tensor* act_a,
                     const sfa_tensor* act_b, const char* acts) {
    SFA_CHECK_ARG(cache_a->dtype == SFA_DTYPE_FP8_E4M3 && cache_b->dtype == SFA_DTYPE_FP8_E4M3,
                  "%s: the cache buffers must be FP8 (e4m3)", who);
    SFA_CHECK_ARG(act_a->dtype == act_b->dtype, "%s: %s must share one dtype", who, acts);
    return SFA_OK;
}

// `who` of a pool call in the messages: the name of its family plus _fp8 / _paged / _paged_fp8
struct Who {
    char s[40];
    Who(const char* base, bool fp8, bool paged) { snprintf(s, sizeof(s), "%s%s%s", base, paged ? "_paged" : "", fp8 ? "_fp8" : ""); }
    Who(const char* base, const SlotPool& pool) : Who(base, pool.fp8, pool.pt.table != nullptr) {}
    operator const char*() const { return s; }
};

// What an FP8 or a paged pool serves: bf16 / f16 at 64 / 80 / 96 / 128, the MFMA instances (no exact-f32 one reads such a
// pool).  An FP8 call asks where its 16-bit sibling checks the head dim, a 16-bit paged call after the sibling's checks.
// fp8_pages_ok (sfa_ring_copy_paged_slots): FP8 pages pass too - the copy moves bytes
int check_pool_served(const char* who, const SlotPool& pool, int dtype, int64_t D, unsigned flags, bool fp8_pages_ok = false) {
    if (dtype == SFA_DTYPE_F32 || (dtype == SFA_DTYPE_FP8_E4M3 && !fp8_pages_ok) || !(D == 64 || D == 80 || D == 96 || D == 128) ||
        (flags & SFA_FLAG_FORCE_GENERIC)) {
        set_error("%s: %s at head dims 64 / 80 / 96 / 128 (got dtype %d, head dim %lld%s)", who,
                  !pool.fp8 ? "a paged pool serves bf16 / f16" : pool.pt.table ? "a paged FP8 pool serves bf16 / f16 activations"
                                                                               : "an FP8 pool serves bf16 / f16 activations",
                  dtype, (long long)D, (flags & SFA_FLAG_FORCE_GENERIC) ? ", SFA_FLAG_FORCE_GENERIC" : "");
        return SFA_ERR_UNSUPPORTED;
    }
    return SFA_OK;
}

// The checks a *_paged_slots call adds (`who`: its name in the messages), made before those of its contiguous sibling:
// the page buffers are descriptors, the table is there, P = shape[2] is a power of two >= 32 (a 32-key ring tile then
// lies inside one page), table_stride >= 1 and both page buffers have one shape.  Then `ring` gets the descriptors the
// sibling's checks and the launchers read: [S, H_kv, Wc = table_stride * P, D] with the pages' pointer and strides.
struct PagedRing {
    sfa_tensor k, v;
    PageTable pt;
};

// fp8_ok: the page buffers may hold FP8 codes (the *_paged_fp8_slots calls, sfa_ring_copy_paged_slots)
int paged_ring(const char* who, const sfa_tensor* page_k, const sfa_tensor* page_v, const int32_t* table, int table_stride,
               int64_t S, PagedRing* ring, bool fp8_ok = false) {
    int st;
    if ((st = check_tensor(page_k, "window_k", fp8_ok)) || (st = check_tensor(page_v, "window_v", fp8_ok))) return st;
    SFA_CHECK_ARG(table != nullptr, "page_table: null device pointer");
    const int64_t P = page_k->shape[2];
    SFA_CHECK_ARG(P >= 32 && (P & (P - 1)) == 0,
                  "%s: the page size (window_k shape[2] = %lld) must be a power of two and at least 32", who, (long long)P);
    SFA_CHECK_ARG(table_stride >= 1, "%s: table_stride (%d) must be at least 1 (Wc = table_stride * P)", who, table_stride);
    if ((st = same_shape(page_k, page_v, "window_k", "window_v"))) return st;
    SFA_CHECK_ARG(page_k->shape[0] >= 1 && page_k->shape[0] < (1ll << 30),
                  "%s: the page buffers need shape[0] = n_pages in [1, 2^30) (got %lld)", who, (long long)page_k->shape[0]);
    ring->k = *page_k, ring->v = *page_v;
    ring->k.shape[0] = ring->v.shape[0] = S;
    ring->k.shape[2] = ring->v.shape[2] = (int64_t)table_stride * P;
    ring->pt = PageTable{table, table_stride, P, page_k->shape[0]};
    return SFA_OK;
}

// The pool of an entry point as its signature names it: all zero for the 16-bit contiguous calls.  pool_of turns it into
// the descriptor of the launchers; of a paged call it makes the checks of paged_ring first, under the call's own name
// (`base` plus the pool's suffix), and replaces the page buffers by the ring descriptors.  S: the slots of the pool
struct PoolIn {
    bool fp8;
    const float* kv_scale;
    bool paged;
    const int32_t* table;
    int table_stride;
};

int pool_of(const char* base, const PoolIn& in, int64_t S, const sfa_tensor** window_k, const sfa_tensor** window_v,
            PagedRing* ring, SlotPool* pool) {
    *pool = SlotPool{in.fp8, in.kv_scale, PageTable{}};
    if (!in.paged) return SFA_OK;
    const int st = paged_ring(Who(base, in.fp8, true), *window_k, *window_v, in.table, in.table_stride, S, ring, in.fp8);
    if (st) return st;
    *window_k = &ring->k, *window_v = &ring->v, pool->pt = ring->pt;
    return SFA_OK;
}

// every host-checkable argument of an attention call over a chunk (sfa_decode_ring_multi*, _tree*, _ragged_slots), at
// the state of the descriptor (a device-state call: the full cache); nothing launches
int check_multi(const RingCall& c) {
    const sfa_tensor *q = c.q, *sink_k = c.sink_k, *sink_v = c.sink_v, *window_k = c.window_k, *window_v = c.window_v;
    const sfa_tensor *k_new = c.k_new, *v_new = c.v_new, *o = c.o;
    const int64_t sink_len = c.sink_len, window_len = c.window_len, write_pos = c.write_pos;
    int st;
    const bool kv8 = c.pool.fp8;            // sfa_decode_ring_ragged_fp8_slots, sfa_decode_ring_ragged_paged_fp8_slots
    const Who who8("decode_ragged", c.pool);
    if ((st = check_device_state(c))) return st;
    if ((st = check_tensor(q, "q")) || (st = check_tensor(o, "o")) || (st = check_tensor(sink_k, "sink_k", kv8)) ||
        (st = check_tensor(sink_v, "sink_v", kv8)) || (st = check_tensor(window_k, "window_k", kv8)) ||
        (st = check_tensor(window_v, "window_v", kv8)) || (st = check_tensor(k_new, "k_new")) ||
        (st = check_tensor(v_new, "v_new")))
        return st;
    if ((st = same_shape(q, o, "q", "o")) || (st = same_shape(sink_k, sink_v, "sink_k", "sink_v")) ||
        (st = same_shape(window_k, window_v, "window_k", "window_v")) || (st = same_shape(k_new, v_new, "k_new", "v_new")))
        return st;
    const int64_t B = q->shape[0], Hq = q->shape[1], n = q->shape[2], D = q->shape[3], Hkv = k_new->shape[1];
    const int64_t Wc = window_k->shape[2];
    const bool pool = c.slots != nullptr;
    if (kv8) {
        if ((st = check_fp8_dtypes(who8, sink_k, window_k, q, k_new, "q and k_new / v_new"))) return st;
    } else
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
    SFA_CHECK_ARG(std::isfinite(c.scale), "scale must be finite");
    SFA_CHECK_ARG(sink_len + window_len + n < (1ll << 30) && B * Hq * n < (1ll << 30) && Wc < (1ll << 30),
                  "problem too large");
    if (kv8) {      // the activations at 2 bytes per element, the cache rows at 1
        if ((st = check_pool_served(who8, c.pool, q->dtype, D, c.flags))) return st;
        if ((st = check_rows16({q, o, k_new, v_new}, 2, 7, "decode_multi: rows of every tensor must be 16-byte aligned")))
            return st;
        return check_rows16({sink_k, sink_v, window_k, window_v}, 1, 7,
                            "decode_multi: rows of every tensor must be 16-byte aligned");
    }
    if ((st = decode_multi_check_head_dim(D, q->dtype))) return st;
    return check_rows16({q, o, sink_k, sink_v, window_k, window_v, k_new, v_new}, dtype_size(q->dtype), 7,
                        "decode_multi: rows of every tensor must be 16-byte aligned");
}

int multi_workspace_and_launch(const RingCall& c) {
    const sfa_tensor* q = c.q;
    const size_t need = decode_multi_workspace(q->shape[0], q->shape[1], c.k_new->shape[1], q->shape[2],
                                               c.sink_len + c.window_len + q->shape[2], q->shape[3], q->dtype);
    const int st = check_workspace("decode_multi", need, true, c.workspace, c.workspace_bytes);
    return st ? st : decode_multi_launch(c);
}

// sfa_decode_ring_multi*.  An empty call still commits where there is something to advance: the shared state with
// B == 0 or H_q == 0, the state rows with H_q == 0 only (no rows: no state to read or advance)
int ring_multi(const RingCall& c) {
    g_err[0] = 0;
    int st;
    if ((st = check_multi(c))) return st;
    const int64_t B = c.q->shape[0], Hq = c.q->shape[1];
    if (B == 0 && c.mode != RingState::Shared) return SFA_OK;
    if (B == 0 || Hq == 0) return c.commit && c.mode != RingState::Host ? ring_commit_dyn_launch(c) : SFA_OK;
    return multi_workspace_and_launch(c);
}

// sfa_decode_ring_tree*: the tree-specific checks come after those of the chunk; a tree call never commits
int ring_tree(const RingCall& c) {
    g_err[0] = 0;
    int st;
    if ((st = check_multi(c))) return st;
    const int64_t n = c.q->shape[2];
    SFA_CHECK_ARG(n <= 64, "decode_tree: a tree chunk holds at most 64 nodes (got n = %lld)", (long long)n);
    SFA_NEED(c.parent, "parent");
    SFA_CHECK_ARG(c.parent_bstride == 0 || (c.parent_bstride >= n && c.parent_bstride < (1ll << 30)),
                  "parent_bstride %lld: 0 (one tree shared by the batch) or >= n = %lld (one row per sequence)",
                  (long long)c.parent_bstride, (long long)n);
    if (c.q->shape[0] == 0 || c.q->shape[1] == 0) return SFA_OK;
    return multi_workspace_and_launch(c);
}

// sfa_decode_ring_ragged_slots / sfa_decode_ring_ragged_tree_slots: every check of the slots call at the full cache;
// q / k_new / v_new / o share shape[0] and T there.  parent and commit_seq are device arrays that may be null: nothing
// of them is checkable on the host
int ring_ragged(const RingCall& c) {
    int st;
    if ((st = check_multi(c))) return st;
    const sfa_tensor* q = c.q;
    SFA_CHECK_ARG(q->shape[0] == 1, "decode_ragged: q / k_new / v_new / o must be packed [1, H, T, D] (got shape[0] = %lld)",
                  (long long)q->shape[0]);
    SFA_CHECK_ARG(q->shape[1] >= 1, "decode_ragged: H_q must be at least 1");
    if (c.pool.pt.table && !c.pool.fp8 &&
        (st = check_pool_served(Who("decode_ragged", c.pool), c.pool, q->dtype, q->shape[3], c.flags)))
        return st;
    const size_t need = c.cu_g ? decode_ragged_group_workspace(c.n_seq, c.n_grp, q->shape[1], c.k_new->shape[1], q->shape[2],
                                                               c.sink_len + c.window_len, q->shape[3], q->dtype)
                               : decode_ragged_workspace(c.n_seq, q->shape[1], c.k_new->shape[1], q->shape[2],
                                                         c.sink_len + c.window_len, q->shape[3], q->dtype);
    if ((st = check_workspace("decode_ragged", need, need != 0, c.workspace, c.workspace_bytes))) return st;
    return decode_ragged_launch(c);
}

// the packed attention entry points, sfa_decode_ring_ragged{,_tree,_fp8,_paged,_paged_fp8}_slots: c as SFA_ATTEND_CALL
// fills it, `in` the pool.  The order of the checks: the pages and table of a paged call, the null device arrays, n_seq,
// then ring_ragged.  grouped (the *_group_paged_slots calls): cu_g / n_grp are checked behind cu_q / n_seq
int ragged_slots(RingCall c, const int32_t* parent, const int32_t* commit_seq, int commit, int32_t* state,
                 const int32_t* slots, const int32_t* cu_q, int n_seq, const PoolIn& in = PoolIn{}, bool grouped = false,
                 const int32_t* cu_g = nullptr, int n_grp = 0) {
    g_err[0] = 0;
    PagedRing ring;
    int st;
    if ((st = pool_of("decode_ragged", in, c.sink_k ? c.sink_k->shape[0] : 1, &c.window_k, &c.window_v, &ring, &c.pool)))
        return st;
    SFA_NEED(state, "state");
    SFA_NEED(slots, "slots");
    SFA_NEED(cu_q, "cu_q");
    SFA_CHECK_ARG(n_seq >= 1, "decode_ragged: n_seq (%d) must be at least 1", n_seq);
    if (grouped) {
        SFA_NEED(cu_g, "cu_g");
        SFA_CHECK_ARG(n_grp >= 1, "decode_ragged: n_grp (%d) must be at least 1", n_grp);
        c.cu_g = cu_g, c.n_grp = n_grp;
    }
    c.commit = commit, c.cu_q = cu_q, c.n_seq = n_seq;
    c.parent = parent, c.commit_seq = commit_seq;
    return ring_ragged(device_state(c, RingState::Rows, state, slots));
}

// every host-checkable argument of sfa_ring_commit*; nothing launches
int check_commit(const RingCall& c) {
    const sfa_tensor *window_k = c.window_k, *window_v = c.window_v, *k_new = c.k_new, *v_new = c.v_new;
    int st;
    const bool kv8 = c.pool.fp8;            // sfa_ring_commit_path_ragged_fp8_slots and its _paged_fp8 form
    const Who who8("ring_commit_ragged", c.pool);
    if ((st = check_tensor(window_k, "window_k", kv8)) || (st = check_tensor(window_v, "window_v", kv8)) ||
        (st = check_tensor(k_new, "k_new")) || (st = check_tensor(v_new, "v_new")))
        return st;
    if ((st = same_shape(window_k, window_v, "window_k", "window_v")) || (st = same_shape(k_new, v_new, "k_new", "v_new")))
        return st;
    SFA_NEED(c.count, "count");
    SFA_NEED(c.state, "state");
    if (kv8) {
        if ((st = check_fp8_dtypes(who8, window_k, window_v, k_new, v_new, "k_new and v_new"))) return st;
    } else
        SFA_CHECK_ARG(k_new->dtype == window_k->dtype, "k_new / v_new and the ring must share one dtype");
    const int64_t n = k_new->shape[2], Wc = window_k->shape[2];
    const bool pool = c.slots != nullptr;
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
    if (kv8) {
        if ((st = check_pool_served(who8, c.pool, k_new->dtype, k_new->shape[3], 0))) return st;
        if ((st = check_rows16({k_new, v_new}, es, 3, "ring_commit: rows of every tensor must be 16-byte aligned"))) return st;
        return check_rows16({window_k, window_v}, 1, 3, "ring_commit: rows of every tensor must be 16-byte aligned");
    }
    SFA_CHECK_ARG(k_new->shape[3] > 0 && (k_new->shape[3] * es) % 16 == 0,
                  "ring_commit: K/V rows must be a multiple of 16 bytes (head dim %lld)", (long long)k_new->shape[3]);
    return check_rows16({window_k, window_v, k_new, v_new}, es, 3, "ring_commit: rows of every tensor must be 16-byte aligned");
}

RingCall commit_call(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                     const sfa_tensor* v_new, const int32_t* count, RingState mode, int32_t* state, const int32_t* slots,
                     void* stream) {
    RingCall c{};
    c.window_k = window_k, c.window_v = window_v, c.k_new = k_new, c.v_new = v_new;
    c.count = count, c.mode = mode, c.state = state, c.slots = slots, c.stream = (hipStream_t)stream;
    return c;
}

// sfa_ring_commit_{dyn,rows,slots}.  The shared state is advanced even for B == 0; without rows there is no state
int ring_commit(const RingCall& c) {
    int st;
    if ((st = check_commit(c))) return st;
    if (c.mode == RingState::Rows && c.k_new->shape[0] == 0) return SFA_OK;
    return ring_commit_dyn_launch(c);
}

// sfa_ring_commit_path_{dyn,rows,slots}
int ring_commit_path(RingCall c, const int32_t* path, int64_t path_bstride) {
    c.path = path, c.path_bstride = path_bstride;
    int st;
    if ((st = check_commit(c))) return st;
    const int64_t n = c.k_new->shape[2];
    SFA_NEED(path, "path");
    SFA_CHECK_ARG(path_bstride == 0 || (path_bstride >= n && path_bstride < (1ll << 30)),
                  "path_bstride %lld: 0 (one path shared by the batch) or >= n = %lld (one row per sequence)",
                  (long long)path_bstride, (long long)n);
    if (c.mode == RingState::Rows && c.k_new->shape[0] == 0) return SFA_OK;
    return ring_commit_dyn_launch(c);
}

// sfa_ring_commit_path_ragged_slots: the checks of sfa_ring_commit_slots on the pack, then its own
int ring_commit_ragged(const RingCall& c) {
    int st;
    if ((st = check_commit(c))) return st;
    SFA_CHECK_ARG(c.k_new->shape[0] == 1, "ring_commit_ragged: k_new / v_new must be packed [1, H_kv, T, D] (got shape[0] = %lld)",
                  (long long)c.k_new->shape[0]);
    if (c.pool.pt.table && !c.pool.fp8 &&
        (st = check_pool_served(Who("ring_commit_ragged", c.pool), c.pool, c.k_new->dtype, c.k_new->shape[3], 0)))
        return st;
    return ring_commit_dyn_launch(c);
}

// the packed commit entry points, sfa_ring_commit_path_ragged{,_fp8,_paged,_paged_fp8}_slots; n_slots: the S of a paged
// pool, whose page buffers do not tell it
int commit_ragged_slots(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                        const sfa_tensor* v_new, const int32_t* count, const int32_t* path, const int32_t* cu_q, int n_seq,
                        int32_t* state, const int32_t* slots, void* stream, const PoolIn& in = PoolIn{}, int n_slots = 0) {
    g_err[0] = 0;
    PagedRing ring;
    SlotPool pool;
    int st;
    if ((st = pool_of("ring_commit_ragged", in, n_slots, &window_k, &window_v, &ring, &pool))) return st;
    SFA_NEED(slots, "slots");
    SFA_NEED(cu_q, "cu_q");
    SFA_CHECK_ARG(n_seq >= 1, "ring_commit_ragged: n_seq (%d) must be at least 1", n_seq);
    RingCall c = commit_call(window_k, window_v, k_new, v_new, count, RingState::Rows, state, slots, stream);
    c.path = path, c.cu_q = cu_q, c.n_seq = n_seq, c.pool = pool;
    return ring_commit_ragged(c);
}

// sfa_ring_fill_varlen (slots null: sequence i -> cache row i of n_seq) and the slot prefills
// sfa_ring_fill_varlen{,_fp8,_paged,_paged_fp8}_slots (pool; `in` names its kind)
int fill_varlen(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v, const int32_t* cu_seqlens,
                int n_seq, int32_t* state, void* stream, const int32_t* slots, bool pool, const PoolIn& in = PoolIn{}) {
    g_err[0] = 0;
    PagedRing ring;
    SlotPool kind;
    int st;
    if ((st = pool_of("ring_fill_varlen", in, sink_k ? sink_k->shape[0] : 1, &window_k, &window_v, &ring, &kind))) return st;
    const bool kv8 = kind.fp8;
    if ((st = check_tensor(sink_k, "sink_k", kv8)) || (st = check_tensor(sink_v, "sink_v", kv8)) ||
        (st = check_tensor(window_k, "window_k", kv8)) || (st = check_tensor(window_v, "window_v", kv8)) ||
        (st = check_tensor(k, "k")) || (st = check_tensor(v, "v")))
        return st;
    if ((st = same_shape(sink_k, sink_v, "sink_k", "sink_v")) ||
        (st = same_shape(window_k, window_v, "window_k", "window_v")) || (st = same_shape(k, v, "k", "v")))
        return st;
    SFA_NEED(cu_seqlens, "cu_seqlens");
    SFA_NEED(state, "state");
    SFA_CHECK_ARG(!pool || slots != nullptr, "slots: null device pointer");
    SFA_CHECK_ARG(n_seq >= 1, "n_seq must be >= 1 (got %d)", n_seq);
    SFA_CHECK_ARG(k->shape[0] == 1, "packed layout: k / v must be [1, H_kv, T, D] (batch dim %lld)", (long long)k->shape[0]);
    const Who who("ring_fill_varlen", kind);
    if (kv8) {      // sfa_ring_fill_varlen_fp8_slots, sfa_ring_fill_varlen_paged_fp8_slots
        if ((st = check_fp8_dtypes(who, sink_k, window_k, k, v, "k and v"))) return st;
    } else
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
    if (kv8) {
        if ((st = check_pool_served(who, kind, k->dtype, D, 0))) return st;
        if ((st = check_rows16({k, v}, es, 7, "ring_fill_varlen: rows of every tensor must be 16-byte aligned")) ||
            (st = check_rows16({sink_k, sink_v, window_k, window_v}, 1, 7,
                               "ring_fill_varlen: rows of every tensor must be 16-byte aligned")))
            return st;
        return ring_fill_varlen_launch(sink_k, sink_v, window_k, window_v, k, v, cu_seqlens, n_seq, state,
                                       (hipStream_t)stream, slots, kind);
    }
    SFA_CHECK_ARG(D > 0 && (D * es) % 16 == 0, "ring_fill_varlen: K/V rows must be a multiple of 16 bytes (head dim %lld)",
                  (long long)D);
    if ((st = check_rows16({sink_k, sink_v, window_k, window_v, k, v}, es, 7,
                           "ring_fill_varlen: rows of every tensor must be 16-byte aligned")))
        return st;
    if (kind.pt.table && (st = check_pool_served(who, kind, k->dtype, D, 0))) return st;
    return ring_fill_varlen_launch(sink_k, sink_v, window_k, window_v, k, v, cu_seqlens, n_seq, state,
                                   (hipStream_t)stream, slots, kind);
}

// sfa_ring_copy_slots: src / dst = {sink_k, sink_v, window_k, window_v} of the two pools.  The device arrays (slots,
// state) are not looked at: skipped pairs are decided by the kernel
int copy_slots(const sfa_tensor* const src[4], const int32_t* src_state, const sfa_tensor* const dst[4],
               int32_t* dst_state, const int32_t* src_slots, const int32_t* dst_slots, int n_pairs, void* stream,
               const SlotPool& src_pool = SlotPool{}, const SlotPool& dst_pool = SlotPool{}) {
    g_err[0] = 0;
    static const char* const names[8] = {"src_sink_k", "src_sink_v", "src_window_k", "src_window_v",
                                         "dst_sink_k", "dst_sink_v", "dst_window_k", "dst_window_v"};
    int st;
    for (int i = 0; i < 8; ++i)
        if ((st = check_tensor(i < 4 ? src[i] : dst[i - 4], names[i], true))) return st;      // FP8 pools: a byte copy
    SFA_NEED(src_state, "src_state");
    SFA_NEED(dst_state, "dst_state");
    SFA_NEED(src_slots, "src_slots");
    SFA_NEED(dst_slots, "dst_slots");
    SFA_CHECK_ARG(n_pairs >= 0, "n_pairs must be >= 0 (got %d)", n_pairs);
    if (n_pairs == 0) return SFA_OK;
    for (int i = 1; i < 8; ++i)
        SFA_CHECK_ARG((i < 4 ? src[i] : dst[i - 4])->dtype == src[0]->dtype,
                      "ring_copy_slots: %s and src_sink_k differ in dtype (the eight buffers must share one)", names[i]);
    const int64_t Hkv = src[2]->shape[1], ns = src[0]->shape[2], Wc = src[2]->shape[2], D = src[2]->shape[3];
    for (int i = 0; i < 8; ++i) {      // both pools [S, Hkv, num_sink or Wc, D]: equal geometry, S of each pool free
        const sfa_tensor* t = i < 4 ? src[i] : dst[i - 4];
        SFA_CHECK_ARG(t->shape[1] == Hkv && t->shape[2] == ((i & 2) ? Wc : ns) && t->shape[3] == D,
                      "ring_copy_slots: %s must be [S, H_kv, %s, D] = [S, %lld, %lld, %lld] in both pools (got [%lld, "
                      "%lld, %lld, %lld])", names[i], (i & 2) ? "Wc" : "num_sink", (long long)Hkv,
                      (long long)((i & 2) ? Wc : ns), (long long)D, (long long)t->shape[0], (long long)t->shape[1],
                      (long long)t->shape[2], (long long)t->shape[3]);
    }
    for (int p = 0; p < 2; ++p) {
        const sfa_tensor* const* b = p ? dst : src;
        const int64_t S = b[0]->shape[0];
        SFA_CHECK_ARG(S >= 1 && S < (1ll << 30) && b[1]->shape[0] == S && b[2]->shape[0] == S && b[3]->shape[0] == S,
                      "pool: the %s sink and window buffers must share shape[0] = S >= 1 (sink %lld / %lld, window %lld "
                      "/ %lld)", p ? "dst" : "src", (long long)S, (long long)b[1]->shape[0], (long long)b[2]->shape[0],
                      (long long)b[3]->shape[0]);
    }
    SFA_CHECK_ARG(Wc >= 1, "the ring needs a capacity of at least one slot");
    const int es = dtype_size(src[0]->dtype);
    SFA_CHECK_ARG(D > 0 && (D * es) % 16 == 0, "ring_copy_slots: K/V rows must be a multiple of 16 bytes (head dim %lld)",
                  (long long)D);
    SFA_CHECK_ARG(ns + Wc < (1ll << 30) && (ns + Wc) * (D * es / 16) < (1ll << 30) && Hkv < (1ll << 30),
                  "problem too large");
    if ((st = check_rows16({src[0], src[1], src[2], src[3], dst[0], dst[1], dst[2], dst[3]}, es, 7,
                           "ring_copy_slots: rows of every tensor must be 16-byte aligned")))
        return st;
    if (src_pool.pt.table && (st = check_pool_served(Who("ring_copy", src_pool), src_pool, src[0]->dtype, D, 0, true)))
        return st;      // FP8 pages: bytes
    return ring_copy_slots_launch(src, src_state, dst, dst_state, src_slots, dst_slots, n_pairs, (hipStream_t)stream,
                                  src_pool, dst_pool);
}

// sfa_ring_export{,_fp8,_paged,_paged_fp8}_slots: the live tokens of the named slots into a pack (`in` names the kind of
// pool).  The device arrays (cu, state, slots, the table) are not looked at
int export_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k, const sfa_tensor* window_v,
                 const sfa_tensor* k_out, const sfa_tensor* v_out, const int32_t* cu_seqlens, int n_seq, const int32_t* state,
                 const int32_t* slots, int32_t* pos_out, void* stream, const PoolIn& in = PoolIn{}) {
    g_err[0] = 0;
    PagedRing ring;
    SlotPool kind;
    int st;
    if ((st = pool_of("ring_export", in, sink_k ? sink_k->shape[0] : 1, &window_k, &window_v, &ring, &kind))) return st;
    const bool kv8 = kind.fp8;
    if ((st = check_tensor(sink_k, "sink_k", kv8)) || (st = check_tensor(sink_v, "sink_v", kv8)) ||
        (st = check_tensor(window_k, "window_k", kv8)) || (st = check_tensor(window_v, "window_v", kv8)) ||
        (st = check_tensor(k_out, "k_out")) || (st = check_tensor(v_out, "v_out")))
        return st;
    if ((st = same_shape(sink_k, sink_v, "sink_k", "sink_v")) ||
        (st = same_shape(window_k, window_v, "window_k", "window_v")) || (st = same_shape(k_out, v_out, "k_out", "v_out")))
        return st;
    SFA_NEED(cu_seqlens, "cu_seqlens");
    SFA_NEED(state, "state");
    SFA_NEED(slots, "slots");
    SFA_CHECK_ARG(n_seq >= 1, "n_seq must be >= 1 (got %d)", n_seq);
    SFA_CHECK_ARG(k_out->shape[0] == 1, "packed layout: k_out / v_out must be [1, H_kv, T, D] (batch dim %lld)",
                  (long long)k_out->shape[0]);
    const Who who("ring_export", kind);
    if (kv8) {      // sfa_ring_export_fp8_slots, sfa_ring_export_paged_fp8_slots
        if ((st = check_fp8_dtypes(who, sink_k, window_k, k_out, v_out, "k_out and v_out"))) return st;
    } else
        SFA_CHECK_ARG(k_out->dtype == sink_k->dtype && k_out->dtype == window_k->dtype,
                      "k_out / v_out and the cache buffers must share one dtype");
    const int64_t Hkv = k_out->shape[1], D = k_out->shape[3], Wc = window_k->shape[2];
    SFA_CHECK_ARG(sink_k->shape[0] >= 1 && sink_k->shape[0] == window_k->shape[0] && sink_k->shape[0] < (1ll << 30),
                  "pool: sink and window buffers must share shape[0] = S >= 1 (sink %lld, window %lld)",
                  (long long)sink_k->shape[0], (long long)window_k->shape[0]);
    SFA_CHECK_ARG(sink_k->shape[1] == Hkv && sink_k->shape[3] == D && window_k->shape[1] == Hkv && window_k->shape[3] == D,
                  "sink / window buffers must be [S, H_kv, *, D] like k_out");
    SFA_CHECK_ARG(Wc >= 1, "the ring needs a capacity of at least one slot");
    const int es = dtype_size(k_out->dtype);
    SFA_CHECK_ARG(D > 0 && (D * es) % 16 == 0, "ring_export: K/V rows must be a multiple of 16 bytes (head dim %lld)",
                  (long long)D);
    SFA_CHECK_ARG(k_out->shape[2] < (1ll << 30) && k_out->shape[2] * (D * es / 16) < (1ll << 30) &&
                      sink_k->shape[2] + Wc < (1ll << 30) && Hkv < (1ll << 30),
                  "problem too large");
    if ((kv8 || kind.pt.table) && (st = check_pool_served(who, kind, k_out->dtype, D, 0))) return st;
    if ((st = check_rows16({k_out, v_out}, es, 7, "ring_export: rows of every tensor must be 16-byte aligned")) ||
        (st = check_rows16({sink_k, sink_v, window_k, window_v}, kv8 ? 1 : es, 7,
                           "ring_export: rows of every tensor must be 16-byte aligned")))
        return st;
    return ring_export_slots_launch(sink_k, sink_v, window_k, window_v, k_out, v_out, cu_seqlens, n_seq, state, slots,
                                    pos_out, (hipStream_t)stream, kind);
}

}  // namespace

// the parameter lists of include/sfa.h and their pass to attend_call / commit_call
#define SFA_ATTEND_PARAMS                                                                                              \
    const sfa_tensor *q, const sfa_tensor *sink_k, const sfa_tensor *sink_v, const sfa_tensor *window_k,               \
        const sfa_tensor *window_v, const sfa_tensor *k_new, const sfa_tensor *v_new, const sfa_tensor *o,             \
        const float *s_aux
#define SFA_ATTEND_CALL \
    attend_call(q, sink_k, sink_v, window_k, window_v, k_new, v_new, o, s_aux, workspace, workspace_bytes, scale, flags, stream)
#define SFA_TAIL_PARAMS void *workspace, size_t workspace_bytes, float scale, unsigned flags, void *stream
#define SFA_COMMIT_PARAMS \
    const sfa_tensor *window_k, const sfa_tensor *window_v, const sfa_tensor *k_new, const sfa_tensor *v_new, const int32_t *count

extern "C" {

int sfa_decode(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o,
               const float* s_aux, SFA_TAIL_PARAMS) {
    RingCall c = attend_call(q, k, v, nullptr, nullptr, nullptr, nullptr, o, s_aux, workspace, workspace_bytes, scale,
                             flags, stream);
    return ring_step(host_state(c, k ? k->shape[2] : 0, 0, 0));
}

int sfa_decode_ring(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                    const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len, const sfa_tensor* o,
                    const float* s_aux, SFA_TAIL_PARAMS) {
    RingCall c = attend_call(q, sink_k, sink_v, window_k, window_v, nullptr, nullptr, o, s_aux, workspace,
                             workspace_bytes, scale, flags, stream);
    return ring_step(host_state(c, sink_len, window_len, 0));
}

int sfa_decode_ring_step(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                         const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                         int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                         const float* s_aux, SFA_TAIL_PARAMS) {
    g_err[0] = 0;
    SFA_CHECK_ARG(k_new != nullptr && v_new != nullptr, "k_new / v_new: null tensor descriptor");
    RingCall c = SFA_ATTEND_CALL;
    return ring_step(host_state(c, sink_len, window_len, write_pos));
}

int sfa_decode_ring_step_dyn(SFA_ATTEND_PARAMS, int32_t* state, SFA_TAIL_PARAMS) {
    g_err[0] = 0;
    SFA_CHECK_ARG(k_new != nullptr && v_new != nullptr, "k_new / v_new: null tensor descriptor");
    RingCall c = SFA_ATTEND_CALL;
    return ring_step(device_state(c, RingState::Shared, state, nullptr));
}

int sfa_decode_ring_step_rows(SFA_ATTEND_PARAMS, int32_t* state, SFA_TAIL_PARAMS) {
    g_err[0] = 0;
    SFA_CHECK_ARG(k_new != nullptr && v_new != nullptr, "k_new / v_new: null tensor descriptor");
    RingCall c = SFA_ATTEND_CALL;
    return ring_step(device_state(c, RingState::Rows, state, nullptr));
}

int sfa_decode_ring_step_slots(SFA_ATTEND_PARAMS, int32_t* state, const int32_t* slots, SFA_TAIL_PARAMS) {
    g_err[0] = 0;
    SFA_CHECK_ARG(k_new != nullptr && v_new != nullptr, "k_new / v_new: null tensor descriptor");
    SFA_NEED(state, "state");
    SFA_NEED(slots, "slots");
    RingCall c = SFA_ATTEND_CALL;
    return ring_step(device_state(c, RingState::Rows, state, slots));
}

size_t sfa_decode_multi_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t n_new, int64_t Nkv, int64_t D,
                                        int dtype) {
    return decode_multi_workspace(B, Hq, Hkv, n_new, Nkv, D, dtype);
}

int sfa_decode_ring_multi(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                          const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                          int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                          const float* s_aux, int commit, SFA_TAIL_PARAMS) {
    RingCall c = SFA_ATTEND_CALL;
    c.commit = commit;
    return ring_multi(host_state(c, sink_len, window_len, write_pos));
}

int sfa_decode_ring_multi_dyn(SFA_ATTEND_PARAMS, int commit, int32_t* state, SFA_TAIL_PARAMS) {
    RingCall c = SFA_ATTEND_CALL;
    c.commit = commit;
    return ring_multi(device_state(c, RingState::Shared, state, nullptr));
}

int sfa_decode_ring_multi_rows(SFA_ATTEND_PARAMS, int commit, int32_t* state, SFA_TAIL_PARAMS) {
    RingCall c = SFA_ATTEND_CALL;
    c.commit = commit;
    return ring_multi(device_state(c, RingState::Rows, state, nullptr));
}

int sfa_decode_ring_multi_slots(SFA_ATTEND_PARAMS, int commit, int32_t* state, const int32_t* slots, SFA_TAIL_PARAMS) {
    g_err[0] = 0;
    SFA_NEED(state, "state");
    SFA_NEED(slots, "slots");
    RingCall c = SFA_ATTEND_CALL;
    c.commit = commit;
    return ring_multi(device_state(c, RingState::Rows, state, slots));
}

size_t sfa_decode_ragged_workspace_bytes(int64_t n_seq, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache,
                                         int64_t D, int dtype) {
    return decode_ragged_workspace(n_seq, Hq, Hkv, T, Nkv_cache, D, dtype);
}

int sfa_decode_ring_ragged_slots(SFA_ATTEND_PARAMS, int commit, int32_t* state, const int32_t* slots,
                                 const int32_t* cu_q, int n_seq, SFA_TAIL_PARAMS) {
    return ragged_slots(SFA_ATTEND_CALL, nullptr, nullptr, commit, state, slots, cu_q, n_seq);
}

int sfa_decode_ring_ragged_tree_slots(SFA_ATTEND_PARAMS, const int32_t* parent, const int32_t* commit_seq, int commit,
                                      int32_t* state, const int32_t* slots, const int32_t* cu_q, int n_seq,
                                      SFA_TAIL_PARAMS) {
    return ragged_slots(SFA_ATTEND_CALL, parent, commit_seq, commit, state, slots, cu_q, n_seq);
}

int sfa_decode_ring_ragged_fp8_slots(SFA_ATTEND_PARAMS, const int32_t* parent, const int32_t* commit_seq, int commit,
                                     int32_t* state, const int32_t* slots, const int32_t* cu_q, int n_seq,
                                     const float* kv_scale, SFA_TAIL_PARAMS) {
    return ragged_slots(SFA_ATTEND_CALL, parent, commit_seq, commit, state, slots, cu_q, n_seq, PoolIn{true, kv_scale});
}

int sfa_decode_ring_tree(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                         const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                         int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                         const float* s_aux, const int32_t* parent, int64_t parent_bstride, SFA_TAIL_PARAMS) {
    RingCall c = SFA_ATTEND_CALL;
    c.parent = parent, c.parent_bstride = parent_bstride;
    return ring_tree(host_state(c, sink_len, window_len, write_pos));
}

int sfa_decode_ring_tree_dyn(SFA_ATTEND_PARAMS, const int32_t* parent, int64_t parent_bstride, int32_t* state,
                             SFA_TAIL_PARAMS) {
    RingCall c = SFA_ATTEND_CALL;
    c.parent = parent, c.parent_bstride = parent_bstride;
    return ring_tree(device_state(c, RingState::Shared, state, nullptr));
}

int sfa_decode_ring_tree_rows(SFA_ATTEND_PARAMS, const int32_t* parent, int64_t parent_bstride, int32_t* state,
                              SFA_TAIL_PARAMS) {
    RingCall c = SFA_ATTEND_CALL;
    c.parent = parent, c.parent_bstride = parent_bstride;
    return ring_tree(device_state(c, RingState::Rows, state, nullptr));
}

int sfa_decode_ring_tree_slots(SFA_ATTEND_PARAMS, const int32_t* parent, int64_t parent_bstride, int32_t* state,
                               const int32_t* slots, SFA_TAIL_PARAMS) {
    g_err[0] = 0;
    SFA_NEED(state, "state");
    SFA_NEED(slots, "slots");
    RingCall c = SFA_ATTEND_CALL;
    c.parent = parent, c.parent_bstride = parent_bstride;
    return ring_tree(device_state(c, RingState::Rows, state, slots));
}

int sfa_ring_commit_dyn(SFA_COMMIT_PARAMS, int32_t* state, void* stream) {
    g_err[0] = 0;
    return ring_commit(commit_call(window_k, window_v, k_new, v_new, count, RingState::Shared, state, nullptr, stream));
}

int sfa_ring_commit_rows(SFA_COMMIT_PARAMS, int32_t* state, void* stream) {
    g_err[0] = 0;
    return ring_commit(commit_call(window_k, window_v, k_new, v_new, count, RingState::Rows, state, nullptr, stream));
}

int sfa_ring_commit_slots(SFA_COMMIT_PARAMS, int32_t* state, const int32_t* slots, void* stream) {
    g_err[0] = 0;
    SFA_NEED(slots, "slots");
    return ring_commit(commit_call(window_k, window_v, k_new, v_new, count, RingState::Rows, state, slots, stream));
}

int sfa_ring_commit_path_dyn(SFA_COMMIT_PARAMS, const int32_t* path, int64_t path_bstride, int32_t* state, void* stream) {
    g_err[0] = 0;
    return ring_commit_path(commit_call(window_k, window_v, k_new, v_new, count, RingState::Shared, state, nullptr, stream),
                            path, path_bstride);
}

int sfa_ring_commit_path_rows(SFA_COMMIT_PARAMS, const int32_t* path, int64_t path_bstride, int32_t* state, void* stream) {
    g_err[0] = 0;
    return ring_commit_path(commit_call(window_k, window_v, k_new, v_new, count, RingState::Rows, state, nullptr, stream),
                            path, path_bstride);
}

int sfa_ring_commit_path_slots(SFA_COMMIT_PARAMS, const int32_t* path, int64_t path_bstride, int32_t* state,
                               const int32_t* slots, void* stream) {
    g_err[0] = 0;
    SFA_NEED(slots, "slots");
    return ring_commit_path(commit_call(window_k, window_v, k_new, v_new, count, RingState::Rows, state, slots, stream),
                            path, path_bstride);
}

int sfa_ring_commit_path_ragged_slots(SFA_COMMIT_PARAMS, const int32_t* path, const int32_t* cu_q, int n_seq,
                                      int32_t* state, const int32_t* slots, void* stream) {
    return commit_ragged_slots(window_k, window_v, k_new, v_new, count, path, cu_q, n_seq, state, slots, stream);
}

int sfa_ring_commit_path_ragged_fp8_slots(SFA_COMMIT_PARAMS, const int32_t* path, const int32_t* cu_q, int n_seq,
                                          int32_t* state, const int32_t* slots, const float* kv_scale, void* stream) {
    return commit_ragged_slots(window_k, window_v, k_new, v_new, count, path, cu_q, n_seq, state, slots, stream,
                               PoolIn{true, kv_scale});
}

int sfa_ring_fill_varlen_fp8_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                   const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                                   const int32_t* cu_seqlens, int n_seq, int32_t* state, const int32_t* slots,
                                   const float* kv_scale, void* stream) {
    return fill_varlen(sink_k, sink_v, window_k, window_v, k, v, cu_seqlens, n_seq, state, stream, slots, true,
                       PoolIn{true, kv_scale});
}

int sfa_decode_ring_ragged_paged_slots(SFA_ATTEND_PARAMS, const int32_t* parent, const int32_t* commit_seq, int commit,
                                       int32_t* state, const int32_t* slots, const int32_t* cu_q, int n_seq,
                                       const int32_t* page_table, int table_stride, SFA_TAIL_PARAMS) {
    return ragged_slots(SFA_ATTEND_CALL, parent, commit_seq, commit, state, slots, cu_q, n_seq,
                        PoolIn{false, nullptr, true, page_table, table_stride});
}

int sfa_ring_commit_path_ragged_paged_slots(SFA_COMMIT_PARAMS, const int32_t* path, const int32_t* cu_q, int n_seq,
                                            int32_t* state, const int32_t* slots, const int32_t* page_table,
                                            int table_stride, int n_slots, void* stream) {
    return commit_ragged_slots(window_k, window_v, k_new, v_new, count, path, cu_q, n_seq, state, slots, stream,
                               PoolIn{false, nullptr, true, page_table, table_stride}, n_slots);
}

int sfa_ring_fill_varlen_paged_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                     const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                                     const int32_t* cu_seqlens, int n_seq, int32_t* state, const int32_t* slots,
                                     const int32_t* page_table, int table_stride, void* stream) {
    return fill_varlen(sink_k, sink_v, window_k, window_v, k, v, cu_seqlens, n_seq, state, stream, slots, true,
                       PoolIn{false, nullptr, true, page_table, table_stride});
}

int sfa_ring_copy_paged_slots(const sfa_tensor* src_sink_k, const sfa_tensor* src_sink_v, const sfa_tensor* src_window_k,
                              const sfa_tensor* src_window_v, const int32_t* src_state, const sfa_tensor* dst_sink_k,
                              const sfa_tensor* dst_sink_v, const sfa_tensor* dst_window_k, const sfa_tensor* dst_window_v,
                              int32_t* dst_state, const int32_t* src_slots, const int32_t* dst_slots, int n_pairs,
                              const int32_t* src_page_table, int src_table_stride, const int32_t* dst_page_table,
                              int dst_table_stride, void* stream) {
    g_err[0] = 0;
    PagedRing sr, dr;
    int st;
    if ((st = paged_ring("ring_copy_paged", src_window_k, src_window_v, src_page_table, src_table_stride,
                         src_sink_k ? src_sink_k->shape[0] : 1, &sr, true)) ||
        (st = paged_ring("ring_copy_paged", dst_window_k, dst_window_v, dst_page_table, dst_table_stride,
                         dst_sink_k ? dst_sink_k->shape[0] : 1, &dr, true)))
        return st;
    SFA_CHECK_ARG(sr.pt.page_size == dr.pt.page_size, "ring_copy_paged: the pools differ in page size (src %lld, dst %lld)",
                  (long long)sr.pt.page_size, (long long)dr.pt.page_size);
    const sfa_tensor* const src[4] = {src_sink_k, src_sink_v, &sr.k, &sr.v};
    const sfa_tensor* const dst[4] = {dst_sink_k, dst_sink_v, &dr.k, &dr.v};
    return copy_slots(src, src_state, dst, dst_state, src_slots, dst_slots, n_pairs, stream, SlotPool{false, nullptr, sr.pt},
                      SlotPool{false, nullptr, dr.pt});
}

int sfa_decode_ring_ragged_paged_fp8_slots(SFA_ATTEND_PARAMS, const int32_t* parent, const int32_t* commit_seq, int commit,
                                           int32_t* state, const int32_t* slots, const int32_t* cu_q, int n_seq,
                                           const int32_t* page_table, int table_stride, const float* kv_scale,
                                           SFA_TAIL_PARAMS) {
    return ragged_slots(SFA_ATTEND_CALL, parent, commit_seq, commit, state, slots, cu_q, n_seq,
                        PoolIn{true, kv_scale, true, page_table, table_stride});
}

size_t sfa_decode_ragged_group_workspace_bytes(int64_t n_seq, int64_t n_grp, int64_t Hq, int64_t Hkv, int64_t T,
                                               int64_t Nkv_cache, int64_t D, int dtype) {
    return decode_ragged_group_workspace(n_seq, n_grp, Hq, Hkv, T, Nkv_cache, D, dtype);
}

int sfa_decode_ring_ragged_group_paged_slots(SFA_ATTEND_PARAMS, const int32_t* commit_seq, int commit, int32_t* state,
                                             const int32_t* slots, const int32_t* cu_q, int n_seq, const int32_t* cu_g,
                                             int n_grp, const int32_t* page_table, int table_stride, SFA_TAIL_PARAMS) {
    return ragged_slots(SFA_ATTEND_CALL, nullptr, commit_seq, commit, state, slots, cu_q, n_seq,
                        PoolIn{false, nullptr, true, page_table, table_stride}, true, cu_g, n_grp);
}

int sfa_decode_ring_ragged_group_paged_fp8_slots(SFA_ATTEND_PARAMS, const int32_t* commit_seq, int commit, int32_t* state,
                                                 const int32_t* slots, const int32_t* cu_q, int n_seq, const int32_t* cu_g,
                                                 int n_grp, const int32_t* page_table, int table_stride,
                                                 const float* kv_scale, SFA_TAIL_PARAMS) {
    return ragged_slots(SFA_ATTEND_CALL, nullptr, commit_seq, commit, state, slots, cu_q, n_seq,
                        PoolIn{true, kv_scale, true, page_table, table_stride}, true, cu_g, n_grp);
}

int sfa_ring_commit_path_ragged_paged_fp8_slots(SFA_COMMIT_PARAMS, const int32_t* path, const int32_t* cu_q, int n_seq,
                                                int32_t* state, const int32_t* slots, const int32_t* page_table,
                                                int table_stride, int n_slots, const float* kv_scale, void* stream) {
    return commit_ragged_slots(window_k, window_v, k_new, v_new, count, path, cu_q, n_seq, state, slots, stream,
                               PoolIn{true, kv_scale, true, page_table, table_stride}, n_slots);
}

int sfa_ring_fill_varlen_paged_fp8_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                         const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                                         const int32_t* cu_seqlens, int n_seq, int32_t* state, const int32_t* slots,
                                         const int32_t* page_table, int table_stride, const float* kv_scale,
                                         void* stream) {
    return fill_varlen(sink_k, sink_v, window_k, window_v, k, v, cu_seqlens, n_seq, state, stream, slots, true,
                       PoolIn{true, kv_scale, true, page_table, table_stride});
}

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

int sfa_ring_copy_slots(const sfa_tensor* src_sink_k, const sfa_tensor* src_sink_v, const sfa_tensor* src_window_k,
                        const sfa_tensor* src_window_v, const int32_t* src_state, const sfa_tensor* dst_sink_k,
                        const sfa_tensor* dst_sink_v, const sfa_tensor* dst_window_k, const sfa_tensor* dst_window_v,
                        int32_t* dst_state, const int32_t* src_slots, const int32_t* dst_slots, int n_pairs,
                        void* stream) {
    const sfa_tensor* const src[4] = {src_sink_k, src_sink_v, src_window_k, src_window_v};
    const sfa_tensor* const dst[4] = {dst_sink_k, dst_sink_v, dst_window_k, dst_window_v};
    return copy_slots(src, src_state, dst, dst_state, src_slots, dst_slots, n_pairs, stream);
}

int sfa_ring_export_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                          const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out,
                          const int32_t* cu_seqlens, int n_seq, const int32_t* state, const int32_t* slots,
                          int32_t* pos_out, void* stream) {
    return export_slots(sink_k, sink_v, window_k, window_v, k_out, v_out, cu_seqlens, n_seq, state, slots, pos_out, stream);
}

int sfa_ring_export_fp8_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                              const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out,
                              const int32_t* cu_seqlens, int n_seq, const int32_t* state, const int32_t* slots,
                              int32_t* pos_out, const float* kv_scale, void* stream) {
    return export_slots(sink_k, sink_v, window_k, window_v, k_out, v_out, cu_seqlens, n_seq, state, slots, pos_out, stream,
                        PoolIn{true, kv_scale});
}

int sfa_ring_export_paged_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out,
                                const int32_t* cu_seqlens, int n_seq, const int32_t* state, const int32_t* slots,
                                int32_t* pos_out, const int32_t* page_table, int table_stride, void* stream) {
    return export_slots(sink_k, sink_v, window_k, window_v, k_out, v_out, cu_seqlens, n_seq, state, slots, pos_out, stream,
                        PoolIn{false, nullptr, true, page_table, table_stride});
}

int sfa_ring_export_paged_fp8_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                    const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out,
                                    const int32_t* cu_seqlens, int n_seq, const int32_t* state, const int32_t* slots,
                                    int32_t* pos_out, const int32_t* page_table, int table_stride, const float* kv_scale,
                                    void* stream) {
    return export_slots(sink_k, sink_v, window_k, window_v, k_out, v_out, cu_seqlens, n_seq, state, slots, pos_out, stream,
                        PoolIn{true, kv_scale, true, page_table, table_stride});
}

// The device arrays (slots, state) are not looked at: skipped pairs are decided by the kernel, as in copy_slots
int sfa_ring_share_paged_slots(const sfa_tensor* src_sink_k, const sfa_tensor* src_sink_v, const int32_t* src_state,
                               const sfa_tensor* dst_sink_k, const sfa_tensor* dst_sink_v, int32_t* dst_state,
                               const int32_t* src_slots, const int32_t* dst_slots, int n_pairs, void* stream) {
    g_err[0] = 0;
    static const char* const names[4] = {"src_sink_k", "src_sink_v", "dst_sink_k", "dst_sink_v"};
    const sfa_tensor* const t[4] = {src_sink_k, src_sink_v, dst_sink_k, dst_sink_v};
    int st;
    for (int i = 0; i < 4; ++i)
        if ((st = check_tensor(t[i], names[i], true))) return st;      // FP8 sinks: a byte copy
    SFA_NEED(src_state, "src_state");
    SFA_NEED(dst_state, "dst_state");
    SFA_NEED(src_slots, "src_slots");
    SFA_NEED(dst_slots, "dst_slots");
    SFA_CHECK_ARG(n_pairs >= 0, "n_pairs must be >= 0 (got %d)", n_pairs);
    if (n_pairs == 0) return SFA_OK;
    for (int i = 1; i < 4; ++i)
        SFA_CHECK_ARG(t[i]->dtype == t[0]->dtype,
                      "ring_share_slots: %s and src_sink_k differ in dtype (the four buffers must share one)", names[i]);
    const int64_t Hkv = t[0]->shape[1], ns = t[0]->shape[2], D = t[0]->shape[3];
    for (int i = 0; i < 4; ++i)
        SFA_CHECK_ARG(t[i]->shape[1] == Hkv && t[i]->shape[2] == ns && t[i]->shape[3] == D,
                      "ring_share_slots: %s must be [S, H_kv, num_sink, D] = [S, %lld, %lld, %lld] in both pools (got [%lld, "
                      "%lld, %lld, %lld])", names[i], (long long)Hkv, (long long)ns, (long long)D, (long long)t[i]->shape[0],
                      (long long)t[i]->shape[1], (long long)t[i]->shape[2], (long long)t[i]->shape[3]);
    for (int p = 0; p < 2; ++p) {
        const int64_t S = t[2 * p]->shape[0];
        SFA_CHECK_ARG(S >= 1 && S < (1ll << 30) && t[2 * p + 1]->shape[0] == S,
                      "pool: the %s sink buffers must share shape[0] = S >= 1 (sink %lld / %lld)", p ? "dst" : "src",
                      (long long)S, (long long)t[2 * p + 1]->shape[0]);
    }
    const int es = dtype_size(t[0]->dtype);
    SFA_CHECK_ARG(D > 0 && (D * es) % 16 == 0, "ring_share_slots: K/V rows must be a multiple of 16 bytes (head dim %lld)",
                  (long long)D);
    SFA_CHECK_ARG(Hkv >= 1 && Hkv < (1ll << 30) && ns * (D * es / 16) < (1ll << 30), "problem too large");
    if ((st = check_rows16({t[0], t[1], t[2], t[3]}, es, 7, "ring_share_slots: rows of every tensor must be 16-byte aligned")))
        return st;
    return ring_share_slots_launch(src_sink_k, src_sink_v, src_state, dst_sink_k, dst_sink_v, dst_state, src_slots,
                                   dst_slots, n_pairs, (hipStream_t)stream);
}

int sfa_pages_copy(const sfa_tensor* window_k, const sfa_tensor* window_v, const int32_t* src_pages,
                   const int32_t* dst_pages, int n_pairs, void* stream) {
    g_err[0] = 0;
    int st;
    if ((st = check_tensor(window_k, "window_k", true)) || (st = check_tensor(window_v, "window_v", true))) return st;
    SFA_CHECK_ARG(n_pairs >= 0, "n_pairs must be >= 0 (got %d)", n_pairs);
    if ((st = same_shape(window_k, window_v, "window_k", "window_v"))) return st;
    SFA_CHECK_ARG(window_k->dtype != SFA_DTYPE_F32, "pages_copy: the page buffers hold bf16, f16 or FP8 (e4m3) (got dtype %d)",
                  window_k->dtype);
    SFA_CHECK_ARG(window_k->shape[0] >= 1 && window_k->shape[0] < (1ll << 30),
                  "pages_copy: the page buffers need shape[0] = n_pages in [1, 2^30) (got %lld)", (long long)window_k->shape[0]);
    if (n_pairs == 0) return SFA_OK;
    SFA_NEED(src_pages, "src_pages");
    SFA_NEED(dst_pages, "dst_pages");
    const int64_t Hkv = window_k->shape[1], P = window_k->shape[2], D = window_k->shape[3];
    const int es = dtype_size(window_k->dtype);
    SFA_CHECK_ARG(D > 0 && (D * es) % 16 == 0, "pages_copy: K/V rows must be a multiple of 16 bytes (head dim %lld)",
                  (long long)D);
    SFA_CHECK_ARG(Hkv < (1ll << 30) && P < (1ll << 30) && Hkv * P < (1ll << 30) && Hkv * P * (D * es / 16) < (1ll << 30),
                  "problem too large");
    if ((st = check_rows16({window_k, window_v}, es, 6, "pages_copy: rows of every tensor must be 16-byte aligned"))) return st;
    return pages_copy_launch(window_k, window_v, src_pages, dst_pages, n_pairs, (hipStream_t)stream);
}

}  // extern "C"
