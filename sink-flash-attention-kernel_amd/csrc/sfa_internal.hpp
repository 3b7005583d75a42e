// Internal launcher declarations shared between the translation units of libsfa.
#pragma once
#include "sfa_common.hpp"

namespace sfa {

// sfa_generic.hip
int fwd_generic(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o, float* lse,
                const float* s_aux, const Problem& p, hipStream_t stream);
// consts (optional, 16-bit tensors with 16-byte aligned rows only): [B, Hq, 2, N] row constants of the wave-specialised
// dK/dV kernel, written in the same pass
int bwd_preprocess(const sfa_tensor* o, const sfa_tensor* d_o, const float* lse, const float* s_aux, float* delta,
                   float* dsaux_part, float* ds_aux, const Problem& p, hipStream_t stream, float* consts = nullptr,
                   float lse_factor = 0.f);
bool bwd_preprocess_vectorised(const sfa_tensor* o, const sfa_tensor* d_o, const Problem& p);   // can it emit consts?
int64_t bwd_preprocess_nblk(int64_t N);
int bwd_generic(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* d_o,
                const float* lse, const float* delta, const sfa_tensor* dq, const sfa_tensor* dk,
                const sfa_tensor* dv, const Problem& p, hipStream_t stream);

// sfa_fwd_mfma.hip
bool fwd_mfma_supported(int dtype, int D);
int fwd_mfma(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o, float* lse,
             const float* s_aux, const Problem& p, hipStream_t stream);

// sfa_bwd_mfma.hip
bool bwd_mfma_supported(int dtype, int D);
bool bwd_mfma_varlen_supported(int dtype, int D);   // packed (cu_seqlens) launches
size_t bwd_mfma_workspace_bytes(const Problem& p, int dtype, unsigned flags);
int bwd_mfma(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* d_o,
             const float* lse, const float* delta, const sfa_tensor* dq, const sfa_tensor* dk,
             const sfa_tensor* dv, void* workspace, const Problem& p, unsigned flags, hipStream_t stream,
             bool consts_ready = false);
// SFA_ERR_UNSUPPORTED (message set) for a call bwd_mfma would refuse, SFA_OK otherwise: asked before anything is launched
int bwd_mfma_refused(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* d_o,
                     const sfa_tensor* dq, const sfa_tensor* dk, const sfa_tensor* dv, const Problem& p);
bool bwd_mfma_wants_consts();   // the default dK/dV kernels read the row constants from the head of the workspace
float bwd_mfma_lse_factor(const Problem& p, unsigned flags);   // ... whose first row is -LSE * this factor (follows the dK/dV kernel choice)

// sfa_decode.hip
struct DecodePlan {
    int splits;          // KV splits per (batch, kv head)
    int keys_per_split;  // multiple of the keys one workgroup iteration covers
    int lpk;             // lanes per key row (power of two)
    int gt;              // q heads of a GQA group processed per pass
    int max_splits;      // upper bound of `splits` over every key count <= the planned one (workspace sizing)
};
// int32 arrival counters of the one-pass decode, at the start of the decode workspace
inline size_t decode_counter_bytes(int64_t B, int64_t Hkv) { return (((size_t)(B * Hkv + 1) * sizeof(int)) + 255) & ~(size_t)255; }
int decode_plan(int64_t B, int64_t Hq, int64_t Hkv, int64_t Nkv, int64_t D, int dtype, DecodePlan* plan);
// keys = rows [0, n1) of (k, v) followed by rows [0, n2) of (k2, v2); k2/v2 may be null when n2 == 0
int decode_launch(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, int64_t n1, const sfa_tensor* k2,
                  const sfa_tensor* v2, int64_t n2, const sfa_tensor* o, const float* s_aux, void* workspace,
                  float scale, const DecodePlan& plan, hipStream_t stream, const sfa_tensor* k_new = nullptr,
                  const sfa_tensor* v_new = nullptr, int new_slot = -1, int* dyn_state = nullptr,
                  bool one_pass = false, bool state_rows = false,    // state_rows: dyn_state = per-sequence rows [B][4]
                  const int32_t* slots = nullptr);   // slot call: row b of q works on row slots[b] of the cache and the state

// sfa_decode_multi.hip: several new tokens over the sink + ring cache (sfa_decode_ring_multi); arguments already checked
int decode_multi_check_head_dim(int64_t D, int dtype);
size_t decode_multi_workspace(int64_t B, int64_t Hq, int64_t Hkv, int64_t n_new, int64_t Nkv, int64_t D, int dtype);
int decode_multi_launch(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                        const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len, int64_t write_pos,
                        const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux,
                        int commit, void* workspace, float scale, unsigned flags, hipStream_t stream,
                        int32_t* state = nullptr,    // dyn: sink_len / window_len = the full cache, write_pos = 0
                        bool rows = false,           // state = per-sequence rows [B][4] (sfa_decode_ring_multi_rows)
                        const int32_t* parent = nullptr,   // tree chunk (sfa_decode_ring_tree*, n <= 64, no commit)
                        int64_t parent_bstride = 0,
                        const int32_t* slots = nullptr);   // slot call (rows): the buffers are a pool, B = q's rows

// sfa_decode_ring_ragged_slots: a packed [1, H, T, D] step over a pool (sequence i = rows [cu_q[i], cu_q[i + 1]) on slot
// slots[i]); arguments already checked.  Workspace: partials for T packed rows plus the tables of the preparation launch
size_t decode_ragged_workspace(int64_t n_seq, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache, int64_t D, int dtype);
int decode_ragged_launch(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                         const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                         const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit, int32_t* state,
                         const int32_t* slots, const int32_t* cu_q, int n_seq, void* workspace, float scale,
                         unsigned flags, hipStream_t stream);

// sfa_ring_commit_dyn / _rows: store clamp(count, 0, n) chunk tokens into the ring at the device state, then advance it
int ring_commit_dyn_launch(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                           const sfa_tensor* v_new, const int32_t* count, int32_t* state, hipStream_t stream,
                           bool rows = false, const int32_t* path = nullptr,   // path: sfa_ring_commit_path_*
                           int64_t path_bstride = 0, const int32_t* slots = nullptr);   // slots: sfa_ring_commit*_slots
// sfa_ring_fill_varlen: per-sequence prefill placement of a packed K/V into [n_seq, Hkv, *, D] buffers + state rows
int ring_fill_varlen_launch(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                            const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v, const int32_t* cu,
                            int n_seq, int32_t* state, hipStream_t stream,
                            const int32_t* slots = nullptr);   // slots: sequence i -> row slots[i] of a pool

}  // namespace sfa
