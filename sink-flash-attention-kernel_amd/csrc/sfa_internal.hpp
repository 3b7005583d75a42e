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
                   float* dsaux_part, float* ds_aux, const Problem& p, hipStream_t stream, float* consts,
                   float lse_factor);
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
             bool consts_ready);
// SFA_ERR_UNSUPPORTED (message set) for a call bwd_mfma would refuse, SFA_OK otherwise: asked before anything is launched
int bwd_mfma_refused(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* d_o,
                     const sfa_tensor* dq, const sfa_tensor* dk, const sfa_tensor* dv, const Problem& p);
bool bwd_mfma_wants_consts();   // the default dK/dV kernels read the row constants from the head of the workspace
float bwd_mfma_lse_factor(const Problem& p, unsigned flags);   // ... whose first row is -LSE * this factor (follows the dK/dV kernel choice)

// One call on the sink + ring cache, as every launcher below takes it: named fields, a part that a call does not have is
// null / zero.  An entry point of sfa_api.hip fills the fields its signature provides; the arguments are checked there.
// A paged pool (the *_paged_slots calls): the ring buffers are pages [n_pages, H_kv, P, D] and table[s * stride + j]
// (device int32) names the page of ring slots [j P, (j + 1) P) of slot s; Wc = stride * P.  The API passes the launchers
// ring descriptors that read [S, H_kv, Wc, D] with the pages' pointer and strides, so that every geometry read stays
// where it is; table == null: a contiguous pool.
struct PageTable {
    const int32_t* table;
    int64_t stride, page_size, n_pages;
};

// The slot pool of a packed call (and of the slot prefill and copy), beyond its buffers: the launchers below take it as
// one value, all zero for a 16-bit contiguous pool and for every call that is not on a pool.
// fp8 (the *_fp8_slots calls): the cache buffers hold e4m3fn codes, one byte per element against the 2 of the
// activations; kv_scale = device float [2][H_kv], row 0 K and row 1 V, null = all ones.  Read by the kernels only.
// pt.table set (the *_paged_slots calls): window_k / window_v are the descriptors described at PageTable.
// Both (the *_paged_fp8_slots calls): the pages hold codes
struct SlotPool {
    bool fp8;
    const float* kv_scale;
    PageTable pt;
};

enum class RingState {
    Host,     // {sink_len, window_len, write_pos} below are the state
    Shared,   // `state` = device {sink_len, window_len, write_pos}, one row for the whole batch (the *_dyn calls)
    Rows,     // `state` = device rows [B][4] {sink_len, window_len, write_pos, seen}, one per sequence (*_rows, *_slots)
};
struct RingCall {
    // q / o [B, H_q, n, D], the cache buffers [B or S, H_kv, ns or Wc, D], the chunk k_new / v_new [B, H_kv, n, D].
    // sfa_decode has one key segment: sink_k / sink_v with window_len = 0
    const sfa_tensor *q, *sink_k, *sink_v, *window_k, *window_v, *k_new, *v_new, *o;
    const float* s_aux;
    float scale;
    unsigned flags;
    hipStream_t stream;
    void* workspace;
    size_t workspace_bytes;
    int commit;                  // store the chunk and advance the state after the attention (with `parent`: packed calls only)
    RingState mode;
    // Host: the state.  Shared / Rows: the FULL cache (every sink row, every ring slot, write_pos 0) - launch geometry
    // and workspace cover every fill level, each workgroup reads its row of `state` and replans
    int64_t sink_len, window_len, write_pos;
    int32_t* state;
    // slot call (Rows): the buffers are a pool of S rows, batch row b (sequence i of a pack) works on cache row and
    // state row slots[b]; a value outside [0, S) marks an inactive row
    const int32_t* slots;
    // tree chunk (n <= 64): parent[b * parent_bstride + u] in [-1, u); stride 0 = one tree shared by the batch
    const int32_t* parent;
    int64_t parent_bstride;
    // path commit: chunk token path[b * path_bstride + j] is the j-th one stored
    const int32_t* path;
    int64_t path_bstride;
    const int32_t* count;        // commit calls: clamp(count, 0, n) tokens are stored (one value; Rows: B); null = all n
    // packed call: q / k_new / v_new / o are [1, H, T, D], sequence i = rows [cu_q[i], cu_q[i + 1]) on slot slots[i]
    const int32_t* cu_q;
    int n_seq;
    // packed call with per-sequence commit: with `commit`, sequence i is stored and advanced iff commit_seq[i] != 0
    // (null: every sequence).  In a packed call `parent` is [T], packed like q, with sequence-local entries, and a
    // packed commit (cu_q set) takes `path` [T] and `count` [n_seq] the same way
    const int32_t* commit_seq;
    // packed call on a paged pool with fork groups (the *_group_paged_slots calls): group g = the consecutive sequences
    // [cu_g[g], cu_g[g + 1]) of the pack; device offsets, read by the kernels only.  Null: no groups
    const int32_t* cu_g;
    int n_grp;
    SlotPool pool;              // packed calls: the kind of pool the slots belong to (every other call: zero)
};

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
// one query per row: keys = rows [0, sink_len) of the sink buffers followed by rows [0, window_len) of the ring; with
// k_new / v_new the kernel first stores the token into ring slot write_pos (or the state's)
int decode_launch(const RingCall& c, const DecodePlan& plan);

// sfa_decode_multi.hip: several new tokens over the sink + ring cache; arguments already checked
int decode_multi_check_head_dim(int64_t D, int dtype);
size_t decode_multi_workspace(int64_t B, int64_t Hq, int64_t Hkv, int64_t n_new, int64_t Nkv, int64_t D, int dtype);
int decode_multi_launch(const RingCall& c);      // sfa_decode_ring_multi* / sfa_decode_ring_tree*

// sfa_decode_ring_ragged_slots / sfa_decode_ring_ragged_tree_slots.  Workspace: partials for T packed rows plus the tables of the preparation launch
size_t decode_ragged_workspace(int64_t n_seq, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache, int64_t D, int dtype);
int decode_ragged_launch(const RingCall& c);
// the same with fork groups (c.cu_g): the ungrouped workspace plus the group partials and the group tables; 0 where no
// grouped instance exists (fp32, head dims other than 64 / 80 / 96 / 128)
size_t decode_ragged_group_workspace(int64_t n_seq, int64_t n_grp, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache,
                                     int64_t D, int dtype);

// sfa_ring_commit*: store clamp(count, 0, n) chunk tokens into the ring at the device state, then advance it
int ring_commit_dyn_launch(const RingCall& c);
// sfa_ring_fill_varlen: per-sequence prefill placement of a packed K/V into [n_seq, Hkv, *, D] buffers + state rows;
// slots (null: sequence i -> cache row i): sequence i -> row slots[i] of a pool
// pool (with slots only): FP8 buffers take k / v in 16 bits and quantise the rows as they are stored, pages are stored
// through the table
int ring_fill_varlen_launch(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                            const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v, const int32_t* cu,
                            int n_seq, int32_t* state, hipStream_t stream, const int32_t* slots, const SlotPool& pool);
// sfa_ring_copy_slots: src / dst = {sink_k, sink_v, window_k, window_v} of the two pools (the same pool: a fork); pair i
// copies the live rows and the state row of slot src_slots[i] into slot dst_slots[i].  The pools are both paged or both
// contiguous; the copy moves bytes, so of a pool it reads pt alone
int ring_copy_slots_launch(const sfa_tensor* const src[4], const int32_t* src_state, const sfa_tensor* const dst[4],
                           int32_t* dst_state, const int32_t* src_slots, const int32_t* dst_slots, int n_pairs,
                           hipStream_t stream, const SlotPool& src_pool, const SlotPool& dst_pool);
// sfa_ring_export_slots: the live tokens of slot slots[i], in token order, into rows [cu[i], cu[i + 1]) of the pack
// k_out / v_out [1, Hkv, T, D], zeros in every other row; pos_out (optional, [T]): the position of each row, -1 on zeroed
// rows.  Reads the pool, writes the pack alone.  pool: FP8 buffers are read into the pack's 16-bit dtype by the reading
// rule, pages are read through the table
int ring_export_slots_launch(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                             const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out, const int32_t* cu,
                             int n_seq, const int32_t* state, const int32_t* slots, int32_t* pos_out, hipStream_t stream,
                             const SlotPool& pool);
// sfa_ring_share_paged_slots: the live sink rows and the state row of slot src_slots[i] into slot dst_slots[i]; no ring
int ring_share_slots_launch(const sfa_tensor* src_sink_k, const sfa_tensor* src_sink_v, const int32_t* src_state,
                            const sfa_tensor* dst_sink_k, const sfa_tensor* dst_sink_v, int32_t* dst_state,
                            const int32_t* src_slots, const int32_t* dst_slots, int n_pairs, hipStream_t stream);
// sfa_pages_copy: page src_pages[i] onto page dst_pages[i] of the page buffers [n_pages, Hkv, P, D], K and V, as bytes
int pages_copy_launch(const sfa_tensor* window_k, const sfa_tensor* window_v, const int32_t* src_pages,
                      const int32_t* dst_pages, int n_pairs, hipStream_t stream);

}  // namespace sfa
