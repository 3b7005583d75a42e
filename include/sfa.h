/*
 * sfa.h -- C ABI of libsfa.so: MI355X (gfx950) sink flash attention.
 *
 * This is the drop-in boundary for the hot path of
 * RulinShao/sink-flash-attention-kernel.  Each entry point replaces one Triton
 * launch site (plus the eager PyTorch epilogue next to it) of the reference;
 * citations are <file>:<line> relative to the reference repository.
 *
 *   sfa_fwd      replaces  sink_attention/sink_flash_attention.py:537-554
 *                          (_sink_flash_attn_fwd_kernel, :93-194)
 *   sfa_bwd      replaces  sink_attention/sink_flash_attention.py:581-665
 *                          (Delta at :582, _sink_flash_attn_bwd_dkdv_kernel :256-364,
 *                           _sink_flash_attn_bwd_dq_kernel :371-484, the GQA group sum
 *                           :648-651 and ds_aux :658-665)
 *   sfa_decode   replaces  sink_attention/decode_kernel.py:175-226
 *                          (_decode_split_kv_kernel :28-113 and the PyTorch phase-2
 *                           reduction :201-226)
 *
 * Conventions
 *   - Plain C: pointers, sizes, ints.  No torch / C++ types cross the boundary.
 *   - The library never allocates or frees device memory and never synchronises.  The caller owns every
 *     buffer (outputs and workspaces included) and passes DEVICE pointers.
 *   - Every launch goes to the hipStream_t passed as `stream` (void* here so the
 *     header needs no HIP include); the caller makes the right device current.  One documented exception, opt-in per
 *     call: with SFA_FLAG_BWD_OVERLAP sfa_bwd may put its dQ kernel on a library-owned side stream (see the flag).
 *   - Re-entrant.  Mutable state inside the library, all of it listed here: the thread-local error / path strings; a
 *     per-kernel bitmask of the devices whose dynamic-LDS attribute has been set (atomic OR, idempotent); and, only
 *     for callers that pass SFA_FLAG_BWD_OVERLAP, one side stream + two events per (calling thread, device), created
 *     at that thread's first overlapped sfa_bwd on the device and destroyed when the thread ends.  Nothing else
 *     survives a call.  A RELEASE build reads no environment variable and ignores sfa_debug_set_variant: the SFA_*
 *     tuning knobs and the A/B variants exist in -DSFA_AB development builds only (tools/ab.py, tools/build_ab.sh).
 *   - Return value: 0 = ok, <0 = SFA_ERR_* (argument / support problem, nothing
 *     was launched), >0 = a hipError_t from a launch.
 *   - Tensors are described by sfa_tensor: 4-D [B, H, N, D] with strides in
 *     ELEMENTS.  Any B/H/N strides are accepted (so a [B, N, H, D] activation can be
 *     passed as a permuted view without a copy); the D stride must be 1.
 */
#ifndef SFA_H
#define SFA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFA_ABI_VERSION 2

/* element types of q/k/v/o/do/dq/dk/dv (all tensors of one call share one dtype) */
#define SFA_DTYPE_F32 0
#define SFA_DTYPE_F16 1
#define SFA_DTYPE_BF16 2
/* OCP e4m3fn (not fnuz), one byte per element: legal ONLY on the four cache buffers of the *_fp8_slots calls and on the
 * eight buffers of sfa_ring_copy_slots; every other entry point answers it with "<name>: unknown dtype 3". */
#define SFA_DTYPE_FP8_E4M3 3

#define SFA_OK 0
#define SFA_ERR_INVALID_ARGUMENT (-1)  /* null pointer, shape mismatch, bad stride ...   */
#define SFA_ERR_UNSUPPORTED (-2)       /* e.g. head dim beyond what any kernel handles   */
#define SFA_ERR_WORKSPACE (-3)         /* workspace too small / null                      */

/* flags */
#define SFA_FLAG_FORCE_GENERIC 0x1u /* use the exact-f32 generic kernels even when an MFMA kernel exists */
/* 0x2u was SFA_FLAG_BWD_SPILL_DS in ABI revisions before round 2 (dS saved by the dK/dV kernel, dQ as a GEMM over it:
 * break-even against 7 GB of workspace, removed).  The bit is accepted and ignored. */
/* sfa_decode*: one launch instead of two.  The last KV split of a (batch, KV head) to finish folds the split partials
 * itself (atomic arrival counters).  Contract: the caller OWNS the workspace across calls and zero-initialised its FIRST
 * align256((B * Hkv + 1) * 4) bytes once; the kernel leaves them zero.  No agent-scope fence is involved (the partials are
 * written through and fetched past the per-XCD L2s, the counters are relaxed atomics).  Measured: a gain only where the cache
 * is short enough for ONE split (B = 1, 132 keys: 15.8 vs 19.2 us); at 4100 keys two launches are 2 us faster. */
#define SFA_FLAG_DECODE_ONE_PASS 0x4u
/* sfa_bwd / sfa_bwd_varlen: the dQ and dK/dV kernels are independent; on a SMALL grid (dQ grid below 4 workgroups per
 * CU: batch 1, tensor- or sequence-parallel shards) the dQ kernel is launched on a library-owned side stream of the
 * lowest queue priority, forked from and joined back into `stream` by events, so that it fills the CUs the dK/dV
 * kernel leaves idle (+1.4 ... 17 %).  Capturable (fork / join are event edges), EXCEPT that the side stream itself
 * cannot be created under capture: a thread whose FIRST overlapped call on a device happens while `stream` is being
 * captured runs that call (and every later captured one, until an uncaptured call has created the stream) without
 * overlap.  Every return path behind the fork joins the side stream again.  Without the flag every launch goes to
 * `stream` and the library creates nothing.  sink_attention (Python) sets it by default. */
#define SFA_FLAG_BWD_OVERLAP 0x8u
/* sfa_bwd / sfa_bwd_varlen / sfa_bwd_workspace_bytes: dispatch override of the dK/dV kernel for head dims 64 ... 128
 * (pass the same bits to the workspace query): _ASM = the hand-placed 256-key-block kernel wherever its body serves the
 * shape, _WS = the wave-specialised compiled kernel (128-key blocks).  Neither: the library's rule (hand-placed for
 * dense self-attention batches and for grids that fill the chip).  The parity tests run every backward case under the
 * rule AND with the hand-placed kernel forced. */
#define SFA_FLAG_BWD_DKDV_ASM 0x10u
#define SFA_FLAG_BWD_DKDV_WS 0x20u
/* sfa_decode_ring_ragged_slots: admit new sequences in the call.  A sequence of the pack whose slot is active and whose
 * state row has seen == 0 (read on the device) is taken from position 0: its cache is empty whatever the other three
 * state fields hold, the first min(n_i, num_sink) tokens of its chunk are its sinks, and a commit places the chunk as
 * sfa_ring_fill_varlen_slots does.  Every other sequence of the pack, and every call without the flag, is unchanged.
 * Other entry points ignore the bit.  See the packed ragged step below. */
#define SFA_FLAG_RAGGED_ADMIT 0x40u

/* Accepted strides.  All strides are >= 0 element counts (0 = broadcast) held as int64; the base pointer and every
 * stride of a decode / prefill-MFMA operand are multiples of 16 bytes.
 *   stride[0] (batch, or slot of a pool): any int64 value.  Every kernel family forms `index * stride[0]` in 64 bits, so
 *     a batch or slot may start past 2^31 elements / 4 GiB (a slot pool at Hkv 8, W 4096, D 128 does from slot 512 on).
 *   stride[1] (head): generic (fp32-math), decode and cache kernels: any int64 value.  The MFMA prefill paths
 *     (sfa_fwd / sfa_bwd and the packed forms, 16-bit dtypes) need stride[1] * 2 < 2^32 bytes on every operand: their
 *     hand-placed kernels carry the head stride as a 32-bit byte count.
 *   stride[2] (row): the MFMA prefill paths address rows through 32-bit buffer offsets and need
 *     (N + 320) * stride[2] * 2 + 512 < 2^32 - 65536 in the forward, (N + 1280) * ... in the backward (N = shape[2]).
 * An operand outside the MFMA limits (or with rows not 16-byte aligned) is not an error for sfa_fwd / sfa_bwd with
 * N_q == N_kv: the call runs the generic kernels (sfa_last_path() says "fwd_generic_f32math" / "bwd_generic_f32math").
 * The packed calls and N_q != N_kv have no generic form: they return SFA_ERR_UNSUPPORTED before anything is launched
 * (no output, lse, ds_aux or workspace byte is written). */
typedef struct sfa_tensor {
    void* ptr;         /* device pointer to element [0,0,0,0]                    */
    int64_t shape[4];  /* B, H, N, D                                             */
    int64_t stride[4]; /* in elements; stride[3] must be 1                       */
    int32_t dtype;     /* SFA_DTYPE_*                                            */
    int32_t reserved;
} sfa_tensor;

int sfa_abi_version(void);

/* Thread-local description of the last error returned on this thread ("" if none). */
const char* sfa_last_error(void);

/* Name of the kernel family the last successful call in this PROCESS dispatched to (any
 * thread: autograd runs backward on its own thread), e.g. "fwd_mfma_bf16_d128_nw8_hpw4",
 * "bwd_generic_f32math".  Diagnostic for tests/benchmarks only; racy by design. */
const char* sfa_last_path(void);

/*
 * Measurement hook (bench.py): arm `count` caller-created hipEvent_t handles (null entries are
 * skipped; count = 0 disarms).  While armed, sfa_bwd records on its stream
 *   events[0] at entry, [1] after the preprocess kernels (Delta, ds_aux),
 *   [2] after the dK/dV kernel, [3] after the dQ kernel (= end of sfa_bwd).
 * Process-global and not thread-safe by design: a diagnostic, never used by the op itself.
 */
/* Development hook: in a library built with -DSFA_AB two variants of a kernel body are compiled side by side and
 * `value` picks the one `which` (0 dK/dV, 1 forward, 2 dQ) launches; 3 = workgroup order of the dK/dV kernel, 7 = its
 * ticketed dispatch off - so that tools/ab.py can time them alternately in one process on one device.  A release
 * build stores the value and never reads it: no effect on dispatch (use the SFA_FLAG_BWD_DKDV_* bits for that). */
int sfa_debug_set_variant(int which, int value);
/* Device buffer for the cycle stamps of a diagnostic build (tools/stamps_dkdv.py, tools/stamps_wl.py); unused otherwise. */
int sfa_debug_set_ptr(void* device_buffer);
int sfa_debug_set_stage_events(void* const* events, int count);

/*
 * Forward.  valid(i,j) = (j <= i) && (j < num_sink || j >= i - window + 1)
 *   q,o  [B, Hq, N, D]     k,v [B, Hkv, N, D]   Hq % Hkv == 0
 *        k,v may hold MORE rows than q (N_kv >= N): the queries are then the LAST N positions of the key sequence,
 *        row i sits at position i + N_kv - N (chunked prefill, a sequence-parallel rank with its halo keys
 *        prepended; the reference asserts N_q == N_kv).  MFMA kernels only: SFA_ERR_UNSUPPORTED for fp32 / other
 *        head dims.  dk, dv of sfa_bwd are [B, Hkv, N_kv, D]; lse, dq follow q.
 *   lse  [B, Hq, N] float32, contiguous: log-sum-exp of the scaled scores of the row
 *        INCLUDING the s_aux logit (-inf for a row that sees nothing)
 *   s_aux  nullable, [Hq] float32: per-head extra logit that only enters the denominator
 *   scale  softmax scale (the reference hard-wires 1/sqrt(D), sink_flash_attention.py:505)
 */
int sfa_fwd(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o,
            float* lse, const float* s_aux, int num_sink, int window, float scale,
            unsigned flags, void* stream);

/*
 * Backward.  Inputs q,k,v,o,do,lse,s_aux as produced/consumed by sfa_fwd.
 *   dq [B,Hq,N,D]; dk,dv [B,Hkv,N,D] (already summed over the GQA group);
 *   ds_aux nullable [Hq] float32 (required non-null iff s_aux non-null).
 *   workspace: sfa_bwd_workspace_bytes() bytes of device scratch, 256-byte aligned (N = query rows; the size covers
 *   Delta, the ds_aux partials, the row constants and, where the dK/dV sweep is split into chunks, their partial dK / dV:
 *   the query is an upper bound for every N_kv >= N).  Needs no initialisation, holds no state between calls.
 *   Deterministic: the same inputs give bitwise-identical outputs (partial sums are added in a fixed order).
 */
size_t sfa_bwd_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t N, int64_t D, int dtype,
                               int num_sink, int window, unsigned flags);

int sfa_bwd(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o,
            const sfa_tensor* d_o, const float* lse, const float* s_aux, const sfa_tensor* dq,
            const sfa_tensor* dk, const sfa_tensor* dv, float* ds_aux, void* workspace,
            size_t workspace_bytes, int num_sink, int window, float scale, unsigned flags,
            void* stream);

/*
 * Packed (variable-length) batches, SURVEY.md section 8 f-3.  The reference cannot do this: its boundary hands packed
 * batches back to stock flash attention, which drops s_aux (sink_attention/verl_patch.py:73-93).
 *   q,o,do,dq [1, Hq, T, D]   k,v,dk,dv [1, Hkv, T, D]   lse [Hq, T] float32
 *   cu_seqlens: DEVICE int32 [n_seq + 1], cu[0] = 0, cu[n_seq] = T; sequence i = rows cu[i] .. cu[i+1].  Every
 *   sequence gets its own mask origin (valid(i, j) in its own positions) and its own s_aux term.
 *   max_seqlen: longest sequence (only sizes the grids; an upper bound is fine).
 *   The device array is NOT validated (no host synchronisation): cu must be non-decreasing with cu[0] = 0 and
 *   max_seqlen must not understate the longest sequence, or tiles are silently dropped.  Rows behind cu[n_seq]
 *   (padding) are never written: the caller zero-fills outputs / gradients if it hands in such a pack.
 *   Workspace of sfa_bwd_varlen: sfa_bwd_workspace_bytes(1, Hq, Hkv, T, D, dtype, num_sink, window, 0).
 * 16-bit dtypes and head dims 64 / 80 / 96 / 128 only (sfa_varlen_supported); SFA_ERR_UNSUPPORTED otherwise - the
 * caller can then run the sequences one by one through sfa_fwd / sfa_bwd on strided views.
 */
int sfa_varlen_supported(int dtype, int64_t D);

int sfa_fwd_varlen(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o, float* lse,
                   const float* s_aux, const int32_t* cu_seqlens, int n_seq, int max_seqlen, int num_sink,
                   int window, float scale, unsigned flags, void* stream);

int sfa_bwd_varlen(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o,
                   const sfa_tensor* d_o, const float* lse, const float* s_aux, const sfa_tensor* dq,
                   const sfa_tensor* dk, const sfa_tensor* dv, float* ds_aux, const int32_t* cu_seqlens, int n_seq,
                   int max_seqlen, void* workspace, size_t workspace_bytes, int num_sink, int window, float scale,
                   unsigned flags, void* stream);

/*
 * Single-query decode over every key handed in (no mask; windowing is the cache's job,
 * decode_kernel.py:72-83).
 *   q,o [B, Hq, 1, D]   k,v [B, Hkv, Nkv, D]   s_aux nullable [Hq] float32
 */
/* Monotonic in Nkv: a workspace sized for Nkv serves every call with the same (B, Hq, Hkv, D, dtype) and FEWER keys
 * (a ring cache sizes it once for num_sink + window_size and steps through every fill level). */
size_t sfa_decode_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t Nkv, int64_t D,
                                  int dtype);

int sfa_decode(const sfa_tensor* q, const sfa_tensor* k, const sfa_tensor* v, const sfa_tensor* o,
               const float* s_aux, void* workspace, size_t workspace_bytes, float scale,
               unsigned flags, void* stream);

/*
 * Decode over a sink + sliding-window KV cache WITHOUT linearising it.  Replaces the
 * get_kv() torch.cat copies of sink_attention/cache.py:185-216 followed by sink_decode_attention: the kernel reads
 * rows [0, sink_len) of the sink buffer and rows [0, window_len) of the window ring in place (softmax does not care
 * about key order, so a wrapped ring needs no reordering).
 *   sink_k/v   [B, Hkv, num_sink, D]     sink_len   <= num_sink   valid rows
 *   window_k/v [B, Hkv, window_size, D]  window_len <= window_size valid slots (all of them once the ring is full)
 *   workspace: sfa_decode_workspace_bytes(B, Hq, Hkv, sink_len + window_len, D, dtype)
 */
int sfa_decode_ring(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                    const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                    const sfa_tensor* o, const float* s_aux, void* workspace, size_t workspace_bytes,
                    float scale, unsigned flags, void* stream);

/*
 * One generation step on the sink + ring cache in ONE pass: store the new token's K/V [B, Hkv, 1, D] into ring slot
 * `write_pos` AND attend q over the cache as it is after that store.  Replaces SinkCacheLayer.update()'s slot write +
 * torch.cat linearisation (sink_attention/cache.py:129-216) followed by sink_decode_attention.
 *   window_len: valid ring slots AFTER the append (min(old + 1, window_size)); 0 <= write_pos < window_len.
 *   The slot's previous content (the evicted token) is never read; the caller advances write_pos / window_len.
 *   workspace: sfa_decode_workspace_bytes(B, Hq, Hkv, sink_len + window_len, D, dtype)
 */
int sfa_decode_ring_step(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                         const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                         int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                         const float* s_aux, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                         void* stream);

/*
 * The same step with the cache state on the DEVICE, so that a whole generation step (all layers) can be captured
 * into a hipGraph and replayed without host work: `state` = int32 {sink_len, window_len, write_pos}.  The call stores
 * k_new / v_new into slot write_pos, attends over sink rows [0, sink_len) and ring slots [0, min(window_len + 1,
 * window_size)) and then advances the state (window_len saturates at window_size, write_pos wraps).  Launch geometry
 * does not depend on the state: workspace = sfa_decode_workspace_bytes(B, Hq, Hkv, num_sink + window_size, D, dtype).
 */
int sfa_decode_ring_step_dyn(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                             const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                             const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int32_t* state,
                             void* workspace, size_t workspace_bytes, float scale, unsigned flags, void* stream);

/*
 * n >= 1 NEW tokens over the sink + ring cache in one pass (speculative verify, chunked continuation): what n successive
 * sfa_decode_ring_step calls compute, without committing first.  Replaces SinkCacheLayer.update()'s append-then-
 * linearise of sink_attention/cache.py:129-216 for N_q > 1, which lets a chunk token see keys that the chunk itself
 * evicted.
 *   q, o        [B, Hq, n, D]           k_new, v_new [B, Hkv, n, D]   Hq % Hkv == 0
 *   sink_k/v    [B, Hkv, num_sink, D]   sink_len <= num_sink valid rows
 *   window_k/v  [B, Hkv, Wc, D]         Wc >= 1 = ring capacity; window_len <= Wc valid slots; write_pos = the slot
 *               the next token goes to (write_pos == window_len until the ring is full, any slot once it is)
 *   sink_len / window_len / write_pos describe the cache BEFORE the chunk.
 * Mask.  Ring slot s has the chronological index r = (s - write_pos + window_len) mod Wc (0 = oldest).  Query t (0 <= t < n)
 * attends to every sink row, to ring slot s iff window_len - r + t <= Wc - 1, and to chunk token u iff u <= t and
 * t - u <= Wc - 1.  Softmax scale `scale`; s_aux (nullable [Hq] float32) enters the denominator only.
 * commit = 0: the cache is not touched (a verify pass: rejected drafts never enter the ring).
 * commit != 0: after every read of the cache (a later launch on `stream`), chunk token t >= n - Wc is stored into ring slot
 *   (write_pos + t) mod Wc: the buffers are then bitwise what n sfa_decode_ring_step calls leave.  The caller advances its
 *   counters: write_pos += n (mod Wc), window_len = min(window_len + n, Wc).
 * Kernels: bf16 / f16 at head dims 64 / 80 / 96 / 128 run on MFMA; fp32 and every other head dim whose row is a
 * multiple of 16 bytes and <= 1 KiB on an exact-f32-accumulate kernel (also with SFA_FLAG_FORCE_GENERIC).  No atomics:
 * the same inputs give bitwise-identical outputs.
 *   Every tensor: 16-byte aligned data pointer and B/H/N strides that are multiples of 16 bytes.
 *   workspace: sfa_decode_multi_workspace_bytes(B, Hq, Hkv, n, sink_len + window_len + n, D, dtype) bytes, 256-byte
 *   aligned, no initialisation, no state between calls.  Monotonic in Nkv for a fixed n_new: a workspace sized for
 *   num_sink + Wc + n serves every fill level.  0 = unsupported head dim / dtype.
 */
size_t sfa_decode_multi_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t n_new, int64_t Nkv, int64_t D,
                                        int dtype);

int sfa_decode_ring_multi(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                          const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                          int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                          const float* s_aux, int commit, void* workspace, size_t workspace_bytes, float scale,
                          unsigned flags, void* stream);

/*
 * sfa_decode_ring_multi with the cache state on the DEVICE, so that a speculative step (verify every layer, accept in
 * device code, commit the accepted prefix) can be captured into a hipGraph and replayed without host integers or a sync.
 *   state: int32 {sink_len, window_len, write_pos} in device memory, the cache BEFORE the chunk.  It must describe a
 *   prefilled cache: sink_len <= num_sink, window_len <= Wc, write_pos == window_len until the ring is full (the kernels
 *   clamp each field into the buffers, so a corrupt state cannot address outside them, but its output is undefined).
 * Same mask, kernels and output as sfa_decode_ring_multi at that state, bitwise: every workgroup reads the state and
 * recomputes the tile / split plan with the host formulas; the grid is sized for the full cache (sink_len = num_sink,
 * window_len = Wc) and the workgroups of splits the state does not plan exit at once.
 * commit = 0: neither the cache nor the state changes.  commit != 0: chunk token t >= n - Wc is stored into ring slot
 *   (write_pos + t) mod Wc after every read of the cache, then (a trailing one-thread launch, after every reader of the
 *   state) write_pos = (write_pos + n) mod Wc, window_len = min(window_len + n, Wc); sink_len is unchanged.
 *   workspace: sfa_decode_multi_workspace_bytes(B, Hq, Hkv, n, num_sink + Wc + n, D, dtype), 256-byte aligned.
 * Every host-checkable argument is checked as in sfa_decode_ring_multi (at the full cache) before anything launches.
 */
int sfa_decode_ring_multi_dyn(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                              const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                              const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit,
                              int32_t* state, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                              void* stream);

/*
 * Commit the accepted prefix of a chunk into the ring, driven by a DEVICE count (the acceptance rule runs on the
 * device; no host sync).  a = clamp(*count, 0, n): chunk tokens t in [max(0, a - Wc), a) are stored into ring slot
 * (write_pos + t) mod Wc, then write_pos = (write_pos + a) mod Wc, window_len = min(window_len + a, Wc); sink_len is
 * unchanged (the cache is prefilled).  Afterwards the buffers and the state are what append() of the first a tokens
 * leaves.  16 bytes per thread; two launches (the copy, then a one-thread advance after every reader of the state).
 *   window_k/v [B, Hkv, Wc, D]   k_new/v_new [B, Hkv, n, D] (n >= 1) in the ring's dtype, rows multiples of 16 bytes,
 *   16-byte aligned.   count: device int32 (one value).   state: as for sfa_decode_ring_multi_dyn.
 */
int sfa_ring_commit_dyn(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                        const sfa_tensor* v_new, const int32_t* count, int32_t* state, void* stream);

/*
 * Per-sequence device state (ragged batches).  The calls below take `state` = int32 [B][4] in device memory, one row
 * {sink_len, window_len, write_pos, seen} per batch row b (row-major, contiguous): the first three fields mean what the
 * shared state of the *_dyn calls means, for row b's slice of the buffers alone; `seen` is the row's token count (the
 * position its next token takes).  The kernels advance `seen` with the row and never read it for attention.  The launch
 * geometry and workspace are those of the shared *_dyn call (the full cache); each row plans from its own state.
 */

/*
 * sfa_decode_ring_step_dyn with per-sequence state: row b stores its token into its own write_pos, attends over its own
 * sink rows [0, sink_len) and ring slots [0, min(window_len + 1, Wc)), then its state advances (seen += 1).  Arguments,
 * checks and workspace as for sfa_decode_ring_step_dyn.  SFA_FLAG_DECODE_ONE_PASS: the grid-level last arriver advances
 * all B rows.
 */
int sfa_decode_ring_step_rows(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                              const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                              const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int32_t* state,
                              void* workspace, size_t workspace_bytes, float scale, unsigned flags, void* stream);

/*
 * sfa_decode_ring_multi_dyn with per-sequence state: batch row b attends with the mask and plan of its own state row
 * (row b of the output is bitwise that of a shared-state call at row b's state).  commit != 0: every row stores all n
 * chunk tokens at its own slots and advances by n (seen += n).  Arguments, checks and workspace as for
 * sfa_decode_ring_multi_dyn.
 */
int sfa_decode_ring_multi_rows(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                               const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                               const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit,
                               int32_t* state, void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                               void* stream);

/*
 * sfa_ring_commit_dyn with per-sequence state and counts: count = device int32 [B].  Row b stores chunk tokens
 * [max(0, a_b - Wc), a_b) with a_b = clamp(count[b], 0, n) into its ring slots (write_pos_b + t) mod Wc, then advances
 * by a_b (seen += a_b): afterwards row b is what append() of its first a_b tokens leaves.  Tensor arguments and checks
 * as for sfa_ring_commit_dyn.
 */
int sfa_ring_commit_rows(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                         const sfa_tensor* v_new, const int32_t* count, int32_t* state, void* stream);

/*
 * Prefill a ragged batch: store the K/V of n_seq packed sequences (the layout sfa_fwd_varlen takes) into per-sequence
 * cache buffers and write their state rows, in one launch (16 bytes per thread, no host sync: capturable).
 *   k, v        [1, Hkv, T, D]   sequence b = rows [cu_seqlens[b], cu_seqlens[b + 1]), length L_b
 *   sink_k/v    [n_seq, Hkv, num_sink, D]   window_k/v [n_seq, Hkv, Wc, D], Wc >= 1, k's dtype, rows multiples of 16
 *               bytes and 16-byte aligned
 *   cu_seqlens  device int32 [n_seq + 1]; read on the device and not validated (as sfa_fwd_varlen); offsets are
 *               clamped into [0, T], so that bad ones cannot address outside the pack.
 * Row b gets the placement of a prefill of its sequence alone: with sl = min(L, num_sink) and r = L - sl, sink row
 * j < sl holds token j; if r <= Wc ring slot s < r holds token sl + s, else slot s holds token L - Wc + s.  Rows and
 * slots beyond those keep their content.  state[b] = {sl, min(r, Wc), r < Wc ? r : 0, L}.
 */
int sfa_ring_fill_varlen(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                         const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                         const int32_t* cu_seqlens, int n_seq, int32_t* state, void* stream);

/*
 * Tree-structured speculative verification (Medusa / EAGLE / SpecInfer style): the n new tokens of a chunk form a
 * forest, verified in one pass that reads the cache once.
 *   parent: device int32, row b's tree at parent + b * parent_bstride, entries u in [0, n) (1 <= n <= 64);
 *           parent_bstride = 0: one tree shared by the batch, else >= n (one row per sequence).
 *   parent[u] in [-1, u): -1 = u hangs directly off the cache (several roots are allowed).  On the device any value
 *           outside [-1, u) reads as -1, so the order is topological and a corrupt tree cannot loop or leave the chunk.
 *   depth[u] = 0 for a root, depth[parent[u]] + 1 otherwise; anc[u] = u and all of its ancestors.
 * Mask.  Query u attends to every sink row; to ring slot s with chronological position c = r - window_len
 * (r = (s - write_pos + window_len) mod Wc, so c in [-window_len, -1]) iff c >= depth[u] - Wc + 1; to chunk token v iff
 * v in anc[u] and depth[u] - depth[v] <= Wc - 1.  Node u thus sees exactly what the last of depth[u] + 1 successive
 * sfa_decode_ring_step calls sees when they append its root-to-u path; parent[u] = u - 1 is the mask of
 * sfa_decode_ring_multi, bit for bit.  s_aux enters the denominator only.
 * Same kernels, plan, partials and reduce as sfa_decode_ring_multi (tree instances of the split kernels derive depth
 * and ancestors in-kernel); no commit: a tree chunk is never stored whole (sfa_ring_commit_path_* stores a path).
 * Arguments, checks and workspace (sfa_decode_multi_workspace_bytes) as for the sfa_decode_ring_multi sibling, plus
 * n <= 64, a non-null parent and a valid parent_bstride, all checked before anything launches.
 */
int sfa_decode_ring_tree(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v, int64_t sink_len,
                         const sfa_tensor* window_k, const sfa_tensor* window_v, int64_t window_len,
                         int64_t write_pos, const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                         const float* s_aux, const int32_t* parent, int64_t parent_bstride, void* workspace,
                         size_t workspace_bytes, float scale, unsigned flags, void* stream);

/* sfa_decode_ring_tree with the shared device state of sfa_decode_ring_multi_dyn (bitwise the host-state call at that
 * state); neither the cache nor the state changes. */
int sfa_decode_ring_tree_dyn(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                             const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                             const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, const int32_t* parent,
                             int64_t parent_bstride, int32_t* state, void* workspace, size_t workspace_bytes,
                             float scale, unsigned flags, void* stream);

/* sfa_decode_ring_tree_dyn with per-sequence state rows [B][4]: row b attends with its own state and its own tree
 * (parent + b * parent_bstride). */
int sfa_decode_ring_tree_rows(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                              const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                              const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, const int32_t* parent,
                              int64_t parent_bstride, int32_t* state, void* workspace, size_t workspace_bytes,
                              float scale, unsigned flags, void* stream);

/*
 * Commit an accepted tree PATH: sfa_ring_commit_dyn / sfa_ring_commit_rows with the j-th stored token taken from chunk
 * row path[b * path_bstride + j] (clamped into [0, n)) instead of row j.  a = clamp(count, 0, n): path tokens
 * j in [max(0, a - Wc), a) go to ring slot (write_pos + j) mod Wc, then the state advances by a (the trailing launch
 * of sfa_ring_commit_dyn).  Afterwards buffers and state are what append() of k_new[:, :, path[:a]] leaves.
 *   path: device int32, path_bstride 0 (one path for the batch) or >= n.  Other arguments as for the siblings.
 */
int sfa_ring_commit_path_dyn(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                             const sfa_tensor* v_new, const int32_t* count, const int32_t* path, int64_t path_bstride,
                             int32_t* state, void* stream);

int sfa_ring_commit_path_rows(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                              const sfa_tensor* v_new, const int32_t* count, const int32_t* path, int64_t path_bstride,
                              int32_t* state, void* stream);

/*
 * Slot-indexed calls (continuous batching).  The cache is a POOL of S slots that outlives any one batch:
 *   sink_k/v [S, Hkv, num_sink, D]   window_k/v [S, Hkv, Wc, D]   state int32 [S][4] (the per-sequence rows above)
 * and a step names the slots it works on: `slots` = device int32 [B].  Everything indexed by the batch row today (q,
 * k_new, v_new, o, count, parent, path) keeps B rows and stays indexed by b; batch row b works on cache row and state row
 * slots[b].  One rule for every call:
 *   - slots[b] outside [0, S) (use -1) marks an INACTIVE row: its o rows are written as zeros, nothing is stored for it
 *     and no state row moves.  Decided on the device (no host sync), so a step captured at a fixed B replays at any
 *     occupancy.
 *   - Equivalence.  Let P[s] be the pool gathered by index_select(0, s) (four buffers and the state).  X_slots(pool,
 *     slots, args) writes for every active b bitwise the o[b] that X_rows(P[slots], args) writes at the same B, and
 *     leaves pool[slots[b]] (buffers and state row) bitwise what X_rows leaves in row b.  Pool rows that no active
 *     batch row names are not touched.  Plan, grid and workspace are those of the rows call for B (not for S): a step
 *     costs what its active rows cost.
 *   - The same slot twice in one call: allowed for calls that write nothing (commit = 0, the tree call); undefined for a
 *     call that stores or advances.  The device array is not validated.
 * Host checks before anything launches, as in the siblings: the cache buffers share shape[0] = S >= 1 ("pool: ..."),
 * q / k_new / v_new / o share shape[0] = B, `slots` is non-null ("slots: null device pointer"), and everything the
 * rows call checks, at the full cache.  State writes stay in the positions of the rows calls (trailing launch; reduce
 * block / last arriver of the single-token step), addressed through slots.  sfa_last_path() names carry "_slots"
 * where the rows calls carry "_rows".
 */

/* sfa_decode_ring_step_rows on a pool (two launches, or one with SFA_FLAG_DECODE_ONE_PASS: the grid's last arriver
 * advances state[slots[b]] of every active b).  Workspace: sfa_decode_workspace_bytes(B, Hq, Hkv, num_sink + Wc, D, dtype). */
int sfa_decode_ring_step_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                               const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                               const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int32_t* state,
                               const int32_t* slots, void* workspace, size_t workspace_bytes, float scale,
                               unsigned flags, void* stream);

/* sfa_decode_ring_multi_rows on a pool (commit 0 / 1).  Workspace: sfa_decode_multi_workspace_bytes(B, Hq, Hkv, n,
 * num_sink + Wc + n, D, dtype). */
int sfa_decode_ring_multi_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                                const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit,
                                int32_t* state, const int32_t* slots, void* workspace, size_t workspace_bytes,
                                float scale, unsigned flags, void* stream);

/* sfa_decode_ring_tree_rows on a pool: row b verifies its tree (parent + b * parent_bstride) against slot slots[b]. */
int sfa_decode_ring_tree_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                               const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                               const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, const int32_t* parent,
                               int64_t parent_bstride, int32_t* state, const int32_t* slots, void* workspace,
                               size_t workspace_bytes, float scale, unsigned flags, void* stream);

/* sfa_ring_commit_rows on a pool: row b (count[b], k_new[b]) stores into the ring of slot slots[b] and advances that
 * state row.  window_k/v [S, Hkv, Wc, D], k_new/v_new [B, Hkv, n, D], count device int32 [B]. */
int sfa_ring_commit_slots(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                          const sfa_tensor* v_new, const int32_t* count, int32_t* state, const int32_t* slots,
                          void* stream);

/* sfa_ring_commit_path_rows on a pool. */
int sfa_ring_commit_path_slots(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                               const sfa_tensor* v_new, const int32_t* count, const int32_t* path, int64_t path_bstride,
                               int32_t* state, const int32_t* slots, void* stream);

/*
 * sfa_ring_fill_varlen into a pool: sequence i of the pack (n_seq of them, slots = device int32 [n_seq]) is placed in
 * slot slots[i] and writes that state row; every other slot keeps buffers and state (a sequence whose slot is outside
 * [0, S) is skipped).  This admits a request while the others keep decoding, and reuses a released slot.  S comes from
 * the buffers; the same slot twice is undefined.
 */
int sfa_ring_fill_varlen_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                               const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                               const int32_t* cu_seqlens, int n_seq, int32_t* state, const int32_t* slots,
                               void* stream);

/*
 * Packed ragged step over a pool (chunked prefill and decode in one call).  The new tokens of n_seq sequences lie back
 * to back, the layout sfa_fwd_varlen and sfa_ring_fill_varlen take:
 *   q, o [1, Hq, T, D]   k_new, v_new [1, Hkv, T, D]   cu_q device int32 [n_seq + 1]   slots device int32 [n_seq]
 *   sink_k/v [S, Hkv, num_sink, D]   window_k/v [S, Hkv, Wc, D]   state int32 [S][4]
 * Sequence i is packed rows [cu_q[i], cu_q[i + 1]) (n_i >= 0 of them) and works on cache row and state row slots[i].
 * cu_q is read on the device and not validated: offsets are clamped into [0, T] and made non-decreasing as
 * sfa_ring_fill_varlen does, so bad offsets cannot address outside the pack.
 *   - Mask: sequence i is attended exactly as sfa_decode_ring_multi with n = n_i at the state of its slot (sinks always;
 *     ring position c iff c in [t - Wc + 1, t]; chunk token u iff u <= t and t - u <= Wc - 1).  n_i > Wc is legal.
 *     s_aux enters the denominator only.
 *   - Inactive rows and padding: the o rows of a sequence whose slot is outside [0, S), of an empty sequence (none) and
 *     of packed rows that no sequence covers (the tail behind cu_q[n_seq] of a step captured at a fixed T) are written
 *     as zeros; nothing is stored or advanced for them.  Decided on the device: a step captured at fixed (T, n_seq)
 *     replays at any mix of lengths and any occupancy.
 *   - commit != 0: after every read of the cache (stream order), token t >= n_i - Wc of sequence i goes to ring slot
 *     (write_pos + t) mod Wc of its slot, and a trailing launch advances each named state row by n_i (seen += n_i).
 *     Buffers and state rows are then bitwise what sfa_ring_commit_slots leaves for the same tokens.  Without
 *     SFA_FLAG_RAGGED_ADMIT sink_len never changes: the call continues sequences that a prefill
 *     (sfa_ring_fill_varlen_slots) has admitted.
 *   - flags & SFA_FLAG_RAGGED_ADMIT: the FIRST chunk of a prompt goes through this call too.  Sequence i is admitting
 *     iff its slot is active and state[slots[i]].seen == 0, decided on the device; sink_len, window_len and write_pos of
 *     such a row are taken as 0.  With nsk = min(n_i, num_sink): query t sees chunk token u iff u <= t and (u < nsk or
 *     t - u <= Wc - 1), the mask of a prefill of these n_i tokens (n_i > Wc + num_sink is legal: the sinks stay visible
 *     behind the window).  commit != 0 leaves buffers and state row bitwise as sfa_ring_fill_varlen_slots does for the
 *     sequence: sink row j < nsk holds token j; with rem = n_i - nsk, ring slot s < rem holds token nsk + s if
 *     rem <= Wc, else slot s holds token n_i - Wc + s; state = {nsk, min(rem, Wc), rem < Wc ? rem : 0, n_i}; rows and
 *     slots the sequence does not reach keep their content.  commit == 0 computes the output over the empty cache and
 *     writes nothing.  n_i == 0 on a fresh slot does nothing.  A first chunk shorter than num_sink pins only its own
 *     tokens as sinks (later tokens go to the ring), so a scheduler gives an admitting chunk at least min(prompt,
 *     num_sink) tokens.  Sequences that are not admitting are bit for bit what they are without the flag; workspace
 *     and launches are the same.
 *   - The same slot twice in one call: undefined with commit, allowed without.
 *   - The output rows of a sequence do not depend on where it lies in the pack or on its neighbours: its split plan is
 *     a function of the call's shape (T, n_seq, heads) and its own (state row, n_i).  No atomics.
 * Work is sized by T, not by n_seq * max n_i: a workgroup is (sequence, 32-row block of its G * n_i rows, KV head,
 * split), at most ceil(G T / 32) + n_seq row blocks, mapped by a one-workgroup preparation launch that reads cu_q only.
 * Host checks before anything launches: q / k_new / v_new / o have shape[0] = 1 and share T; the pool buffers share S;
 * state, slots and cu_q are non-null; n_seq >= 1; strides, alignment, head dim and dtype as for
 * sfa_decode_ring_multi_slots; workspace >= sfa_decode_ragged_workspace_bytes(n_seq, Hq, Hkv, T, num_sink + Wc, D,
 * dtype) bytes, 256-byte aligned (0: unsupported head dim or shape; no GPU needed).  sfa_last_path() names carry
 * "_ragged", then "_admit" with SFA_FLAG_RAGGED_ADMIT, then "_commit".
 * Strides have no upper limit in the packed calls (this one, the _tree / _fp8 / _paged forms, the packed commit, the
 * fills and sfa_ring_copy_slots): every offset is formed in 64 bits on the device, so the pack may lie behind a head
 * stride of 4 GiB or more, a pool behind any slot stride and a page buffer may exceed 4 GiB (n_pages < 2^30).
 */
size_t sfa_decode_ragged_workspace_bytes(int64_t n_seq, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache,
                                         int64_t D, int dtype);

int sfa_decode_ring_ragged_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                 const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                                 const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux, int commit,
                                 int32_t* state, const int32_t* slots, const int32_t* cu_q, int n_seq,
                                 void* workspace, size_t workspace_bytes, float scale, unsigned flags, void* stream);

/*
 * Packed ragged step with draft trees and per-sequence commit (speculative decoding inside the packed step).
 * sfa_decode_ring_ragged_slots with two more device arrays, each of which may be NULL:
 *   parent      int32 [T], packed like q: parent[cu_q[i] + u] is the parent of node u of sequence i as a LOCAL index
 *               in [-1, u); any other value reads as -1 (a root hanging off the cache).  Read on the device after the
 *               clamping of cu_q, at rows [c0_i, c0_i + n_i) only, so a corrupt array cannot leave the pack.
 *   commit_seq  int32 [n_seq]: sequence i is stored and its state row advanced iff commit != 0 && commit_seq[i] != 0.
 *   - parent == NULL: the mask, the kernels and the output bits of sfa_decode_ring_ragged_slots.
 *   - parent != NULL: sequence i is a TREE sequence iff n_i <= 64 and it is not admitting (SFA_FLAG_RAGGED_ADMIT and
 *     seen == 0), decided on the device per workgroup.  A tree sequence is attended exactly as
 *     sfa_decode_ring_tree_slots with n = n_i at its slot's state: sinks always; ring position c iff
 *     c >= depth[u] - Wc + 1; chunk token v iff v is u or an ancestor of u and depth[u] - depth[v] <= Wc - 1.  Every
 *     other sequence (a prompt chunk longer than 64, an admitting sequence) ignores its parent entries and takes the
 *     mask of sfa_decode_ring_ragged_slots, so a scheduler writes u - 1 for chains of at most 64 tokens and may leave
 *     the rest of the array stale.  With parent[t] = local(t) - 1 everywhere o is bit for bit that of
 *     sfa_decode_ring_ragged_slots, and a sequence's o rows do not depend on its place in the pack or its neighbours.
 *   - commit_seq == NULL: all sequences or none, by commit.  Otherwise a sequence with commit_seq[i] == 0 leaves its
 *     buffers and state row untouched (as with commit == 0); a named one is stored with the placement of
 *     sfa_decode_ring_ragged_slots, the admitting placement included.  Draft rows take 0 (their accepted prefix is
 *     stored later by sfa_ring_commit_path_ragged_slots), decode rows and prompt chunks 1.  The bit set on a tree
 *     sequence stores the WHOLE chunk in packed order: defined, and meaningful only for a chain-shaped parent.
 * Plan, grid, workspace (sfa_decode_ragged_workspace_bytes), launches and host checks are those of
 * sfa_decode_ring_ragged_slots.  sfa_last_path(): "decode_tree_{mfma,f32}_..._ragged..." with parent, else
 * "decode_multi_...".
 */
int sfa_decode_ring_ragged_tree_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                      const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                                      const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux,
                                      const int32_t* parent, const int32_t* commit_seq, int commit, int32_t* state,
                                      const int32_t* slots, const int32_t* cu_q, int n_seq, void* workspace,
                                      size_t workspace_bytes, float scale, unsigned flags, void* stream);

/*
 * Packed commit of accepted prefixes / tree paths: k_new / v_new [1, Hkv, T, D] (the pack of the step), count device
 * int32 [n_seq], path device int32 [T] packed like k_new with sequence-local entries (NULL: the identity), cu_q and
 * slots as in the packed step.  For sequence i with a = clamp(count[i], 0, n_i) the j-th stored token is packed row
 * cu_q[i] + clamp(path[cu_q[i] + j], 0, n_i - 1) (row cu_q[i] + j without a path); tokens j in [max(0, a - Wc), a) go
 * to ring slot (write_pos + j) mod Wc of slot slots[i], and a trailing launch advances the state row by a.  Buffers and
 * state row are bitwise what sfa_ring_commit_path_slots (NULL path: sfa_ring_commit_slots) leaves for the sequence
 * passed as a [1, Hkv, n_i, D] chunk.  Nothing happens for inactive slots, empty sequences, a == 0 and rows that no
 * sequence covers.  Not an admission: sink_len never changes.  One 16-byte piece of K and of V per thread over T rows;
 * no workspace.  Host checks before anything launches: k_new / v_new have shape[0] = 1 and share T; count, cu_q, state
 * and slots are non-null; n_seq >= 1; alignment and dtype as for sfa_ring_commit_slots.
 * sfa_last_path(): "ring_commit_path_ragged_slots".
 */
int sfa_ring_commit_path_ragged_slots(const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                                      const sfa_tensor* v_new, const int32_t* count, const int32_t* path,
                                      const int32_t* cu_q, int n_seq, int32_t* state, const int32_t* slots,
                                      void* stream);

/*
 * FP8 (OCP e4m3fn) slot pool: the packed calls on a pool whose four cache buffers hold one byte per element
 * (SFA_DTYPE_FP8_E4M3; rows of D = 64 / 80 / 96 / 128 bytes, 16-byte aligned like every row).  Activations (q, k_new,
 * v_new, o; k / v of the fill) are bf16 or f16, of one dtype T.  An FP8 pool halves the bytes a step reads and the bytes
 * a slot holds.
 *   kv_scale    device float [2][H_kv], row 0 for K and row 1 for V: one static scale per KV head, owned by the caller
 *               (what a calibrated checkpoint carries).  NULL: all ones.  The kernels read it when they run and it is
 *               never read on the host, so an in-place update is seen by the next replay of a captured graph.  No scale
 *               lives in the pool.
 * Storing a 16-bit element x of KV head h, in f32 with one reciprocal per head:
 *     r = 1.0f / scale[h] (IEEE division);  code = e4m3fn_rne(clamp(float(x) * r, -448, 448))
 * The clamp is explicit: overflow saturates to +-448 (codes 0x7e / 0xfe), never NaN.  Inputs are finite; what a NaN
 * becomes is unspecified.  Reading a code of head h gives T(float(code) * scale[h]): one f32 multiply, rounded to
 * nearest even into T.  Two bitwise equalities follow and are what the tests hold the calls to:
 *   - Storage.  Every cache row a storing call writes holds exactly that expression applied to the 16-bit row the same
 *     call writes into a 16-bit pool; every row the 16-bit call leaves alone keeps its bytes; the state rows are equal.
 *   - Read.  o of a packed step on an FP8 pool is bit for bit o of the same step on a 16-bit pool whose buffers hold
 *     T(float(code) * scale): the sink and ring tiles are converted in registers between the global load and the LDS
 *     store, everything after that is the 16-bit kernel.
 * The tokens of a step (k_new / v_new) are attended at 16-bit precision inside that step and at FP8 precision from the
 * next one on, so a prompt admitted in several chunks is not bitwise the prompt admitted in one call.
 *
 * sfa_decode_ring_ragged_fp8_slots: the arguments of sfa_decode_ring_ragged_tree_slots plus kv_scale in front of
 * workspace.  parent == NULL: the plain ragged mask; commit_seq == NULL, commit and SFA_FLAG_RAGGED_ADMIT as there.  A
 * commit quantises as it stores, the admitting placement into the sink rows included.  Workspace:
 * sfa_decode_ragged_workspace_bytes with q's dtype (the partials are f32).  Host checks: those of the 16-bit call in
 * its order, with "decode_ragged_fp8: the cache buffers must be FP8 (e4m3)" (SFA_ERR_INVALID_ARGUMENT) where it
 * compares the dtypes; fp32 activations and head dims outside 64 / 80 / 96 / 128 are SFA_ERR_UNSUPPORTED (there is no
 * exact-f32 instance for an FP8 pool, and SFA_FLAG_FORCE_GENERIC is refused the same way).  sfa_last_path(): the name of
 * the 16-bit call plus "_kvfp8".
 */
int sfa_decode_ring_ragged_fp8_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                     const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                                     const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux,
                                     const int32_t* parent, const int32_t* commit_seq, int commit, int32_t* state,
                                     const int32_t* slots, const int32_t* cu_q, int n_seq, const float* kv_scale,
                                     void* workspace, size_t workspace_bytes, float scale, unsigned flags,
                                     void* stream);

/*
 * sfa_ring_commit_path_ragged_slots into an FP8 ring: the same arguments plus kv_scale in front of stream; k_new /
 * v_new are bf16 or f16, window_k / window_v FP8.  Slots, order and state advance are those of the 16-bit call; each
 * stored row is quantised by the storing rule above (a thread reads 16 bytes = 8 elements and writes 8 bytes).
 * "ring_commit_ragged_fp8: the cache buffers must be FP8 (e4m3)"; sfa_last_path(): "ring_commit_path_ragged_slots_kvfp8".
 */
int sfa_ring_commit_path_ragged_fp8_slots(const sfa_tensor* window_k, const sfa_tensor* window_v,
                                          const sfa_tensor* k_new, const sfa_tensor* v_new, const int32_t* count,
                                          const int32_t* path, const int32_t* cu_q, int n_seq, int32_t* state,
                                          const int32_t* slots, const float* kv_scale, void* stream);

/*
 * sfa_ring_fill_varlen_slots into an FP8 pool: the same arguments plus kv_scale in front of stream; k / v are bf16 or
 * f16, the four pool buffers FP8.  Placement and state rows are those of the 16-bit call, each stored row quantised by
 * the storing rule.  "ring_fill_varlen_fp8: the cache buffers must be FP8 (e4m3)"; sfa_last_path():
 * "ring_fill_varlen_slots_kvfp8".
 */
int sfa_ring_fill_varlen_fp8_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                   const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                                   const int32_t* cu_seqlens, int n_seq, int32_t* state, const int32_t* slots,
                                   const float* kv_scale, void* stream);

/*
 * Copy slots of a pool on the device: the fork of parallel sampling and beam search (one prefilled prompt into n
 * slots), and parking a sequence in a second pool.  Pair i (n_pairs of them) copies slot s = src_slots[i] of the source
 * pool into slot d = dst_slots[i] of the destination pool; src_slots / dst_slots are device int32 [n_pairs].
 *   src_sink_k/v [S_src, Hkv, num_sink, D]   src_window_k/v [S_src, Hkv, Wc, D]   src_state int32 [S_src][4]
 *   dst_sink_k/v [S_dst, Hkv, num_sink, D]   dst_window_k/v [S_dst, Hkv, Wc, D]   dst_state int32 [S_dst][4]
 *   - Pools.  Source and destination may be the same pool (all five pointers equal; the kernel takes src_state ==
 *     dst_state as "the same pool"), or two pools of equal Hkv, num_sink, Wc, D and dtype with S_src and S_dst free.
 *     Pools that overlap in part are undefined.
 *   - What is copied.  The rows the attention kernels would read for the state of s, read with their clamps: sink rows
 *     j < clamp(sink_len, 0, num_sink) and ring slots j < clamp(window_len, 0, Wc) (a ring that is not full copies only
 *     its live slots, a full ring all Wc), all KV heads, and the state row verbatim (4 ints).  Every row keeps its
 *     position, so write_pos means in d what it means in s: any later call on d is bitwise the same call on s.  Rows
 *     and ring slots the source does not reach keep what d held, as sfa_ring_fill_varlen_slots documents for its
 *     placement.  A source with seen == 0 makes d fresh.
 *   - Skipped pairs, decided on the device: s outside [0, S_src), d outside [0, S_dst), s == d in the same pool (the
 *     slots = -1 rule of the slot calls: a launch captured at a fixed n_pairs replays with any number of live pairs).
 *   - Aliasing.  One source may feed many destinations in one call.  Undefined, and the device arrays are not
 *     validated: a destination named twice; in the same pool, a destination that is also a live source.  Beam
 *     reordering therefore never permutes in place: it forks into free slots and releases the dead ones.
 * One launch on `stream`, capturable; no workspace, no allocation, nothing read on the host.  The grid covers the
 * capacity (n_pairs * Hkv * (num_sink + Wc) rows); workgroups past the live rows of their pair leave after the state
 * read, so the bytes moved follow the fill.  Each thread holds several 16-byte pieces of K and of V in flight before its
 * first store; exactly one thread writes dst_state[d], and no workgroup of the launch reads that row.
 * Host checks before anything launches, in this order: null descriptors ("src_sink_k: null tensor descriptor", ...;
 * unit last stride with them); null src_state / dst_state / src_slots / dst_slots; n_pairs < 0 (n_pairs == 0 returns
 * SFA_OK here, without a launch); one dtype across the eight buffers; equal Hkv, num_sink, Wc, D between the pools and
 * one shape[0] >= 1 within each; rows a multiple of 16 bytes and 16-byte aligned.  sfa_last_path(): "ring_copy_slots".
 * FP8 pools: the eight buffers may all be SFA_DTYPE_FP8_E4M3.  The copy stays a byte copy and takes no scales: the
 * codes of a slot mean in d what they mean in s only if the caller keeps EQUAL kv_scale on pools that exchange slots.
 */
int sfa_ring_copy_slots(const sfa_tensor* src_sink_k, const sfa_tensor* src_sink_v, const sfa_tensor* src_window_k,
                        const sfa_tensor* src_window_v, const int32_t* src_state, const sfa_tensor* dst_sink_k,
                        const sfa_tensor* dst_sink_v, const sfa_tensor* dst_window_k, const sfa_tensor* dst_window_v,
                        int32_t* dst_state, const int32_t* src_slots, const int32_t* dst_slots, int n_pairs,
                        void* stream);

/*
 * Paged slot pool: the packed calls on a pool whose RING memory follows the sequence length.  A contiguous pool holds
 * [S, Hkv, Wc, D] per ring buffer whether a slot has 40 tokens or Wc; a paged pool holds pages and a table:
 *   window_k/v  [n_pages, Hkv, P, D]: the ring PAGES, in the pool's dtype (bf16 or f16, head dims 64 / 80 / 96 / 128),
 *               with the strides of the contiguous buffers and the page index where the slot index was.  P = shape[2] is
 *               a power of two and at least 32, so that a 32-slot ring tile lies inside one page.
 *   page_table  device int32 [S][table_stride], owned by the caller like kv_scale.  Entry [s][j] is the page that holds
 *               ring slots [j P, (j + 1) P) of slot s.  The ring capacity is Wc = table_stride * P (the rule: a table
 *               whose rows are longer than Wc / P entries is passed with table_stride >= Wc / P and means that larger
 *               ring; Wc need not be a power of two, Wc = 320 with P = 64 is legal).  The kernels read the table when
 *               they run and the host never reads it: an in-place update is seen by the next replay of a captured graph.
 *   sink_k/v [S, Hkv, num_sink, D] and state int32 [S][4] are those of the contiguous pool; S comes from the sink buffers.
 * Table entries.  An entry e with (unsigned)e >= n_pages is UNMAPPED (-1 by convention):
 *   - a read of a ring tile whose page is unmapped addresses page 0: in bounds; the output of that sequence is
 *     unspecified and no other sequence's output changes;
 *   - a store to a ring slot whose page is unmapped is dropped; the state row still advances as the contiguous call
 *     advances it;
 *   - every page and row address is computed in 64-bit arithmetic.
 * Pages needed are a prefix.  A ring fills from slot 0 upwards until it is full (the prefill placement and the commit
 * both do), so a slot whose ring has held at most r tokens touches table entries 0 .. ceil(min(r, Wc) / P) - 1 only,
 * in reads and in stores.  An allocator maps that prefix before the call that makes the ring reach it and nothing else.
 * One page mapped into two live slots at once is undefined only where a storing call REACHES it (a ring slot the call
 * writes lies in that page), as the same slot twice is.  Reads through two table rows that name one page are defined:
 * that is how a fork shares its prompt (sfa_ring_share_paged_slots, sfa_pages_copy below).
 * Contract.  Let the TWIN be the contiguous pool with window[s, :, j P : (j + 1) P] = pages[table[s][j]], the same
 * sinks and the same state.  Two bitwise equalities, which are what the tests hold the calls to:
 *   - Read.  o of a paged step is bit for bit o of the same call on the twin: a ring tile's address is one wave-uniform
 *     table lookup plus the twin's arithmetic, everything behind the address is the 16-bit kernel.
 *   - Storage.  After a storing call on both pools every mapped page row equals the twin's ring slot, every row the
 *     contiguous call leaves alone keeps its bytes, pages mapped to no slot of the call keep their bytes, and sinks and
 *     state rows are equal.
 * Host checks, before those of the contiguous sibling (which then run in their order, reading Wc = table_stride * P and
 * S for the ring's shape), SFA_ERR_INVALID_ARGUMENT: null page descriptors ("window_k: null tensor descriptor");
 * "page_table: null device pointer"; "<call>: the page size (window_k shape[2] = P) must be a power of two and at least
 * 32"; "<call>: table_stride (n) must be at least 1 (Wc = table_stride * P)"; page buffers of unequal shape ("window_k
 * and window_v differ in shape[i]: ..."); "<call>: the page buffers need shape[0] = n_pages in [1, 2^30) (got n)".  After
 * the sibling's checks: fp32, head dims outside 64 / 80 / 96 / 128 and SFA_FLAG_FORCE_GENERIC are SFA_ERR_UNSUPPORTED
 * ("<call>: a paged pool serves bf16 / f16 at head dims 64 / 80 / 96 / 128 (...)"): there is no exact-f32 instance.
 * <call> is decode_ragged_paged, ring_commit_ragged_paged, ring_fill_varlen_paged or ring_copy_paged.  FP8 pages are
 * served by the *_paged_fp8_slots calls below (and copied by sfa_ring_copy_paged_slots); these three calls refuse them.
 *
 * sfa_decode_ring_ragged_paged_slots: the arguments of sfa_decode_ring_ragged_tree_slots plus (page_table,
 * table_stride) in front of workspace; parent, commit_seq, commit and SFA_FLAG_RAGGED_ADMIT as there.  Workspace:
 * sfa_decode_ragged_workspace_bytes with Nkv_cache = num_sink + Wc.  sfa_last_path(): the name of the contiguous call
 * plus "_paged".
 */
int sfa_decode_ring_ragged_paged_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                       const sfa_tensor* window_k, const sfa_tensor* window_v, const sfa_tensor* k_new,
                                       const sfa_tensor* v_new, const sfa_tensor* o, const float* s_aux,
                                       const int32_t* parent, const int32_t* commit_seq, int commit, int32_t* state,
                                       const int32_t* slots, const int32_t* cu_q, int n_seq, const int32_t* page_table,
                                       int table_stride, void* workspace, size_t workspace_bytes, float scale,
                                       unsigned flags, void* stream);

/*
 * sfa_ring_commit_path_ragged_slots into a paged ring: the same arguments plus (page_table, table_stride, n_slots) in
 * front of stream.  n_slots = S, the rows of `state` and of the table: the contiguous call reads S from the ring buffers,
 * which here hold pages, and this call takes no sink buffers.  sfa_last_path(): "ring_commit_path_ragged_slots_paged".
 */
int sfa_ring_commit_path_ragged_paged_slots(const sfa_tensor* window_k, const sfa_tensor* window_v,
                                            const sfa_tensor* k_new, const sfa_tensor* v_new, const int32_t* count,
                                            const int32_t* path, const int32_t* cu_q, int n_seq, int32_t* state,
                                            const int32_t* slots, const int32_t* page_table, int table_stride,
                                            int n_slots, void* stream);

/* sfa_ring_fill_varlen_slots into a paged pool: the same arguments plus (page_table, table_stride) in front of stream.
 * The state row is written whether or not the ring's pages are mapped.  sfa_last_path(): "ring_fill_varlen_slots_paged". */
int sfa_ring_fill_varlen_paged_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                     const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                                     const int32_t* cu_seqlens, int n_seq, int32_t* state, const int32_t* slots,
                                     const int32_t* page_table, int table_stride, void* stream);

/*
 * sfa_ring_copy_slots between paged pools: the same arguments plus a (page_table, table_stride) pair for each side in
 * front of stream.  Copies the live sink rows, the live ring slots j < clamp(window_len, 0, Wc) through both tables (slot
 * j is read from row j mod P of the source's page and stored into row j mod P of the destination's) and the state row.
 * Source and destination are one pool (all pointers equal, the tables included) or two pools of equal geometry, P
 * included ("ring_copy_paged: the pools differ in page size (src a, dst b)"); n_pages of each is free.  The caller maps
 * the destination's pages for the source's fill first (the prefix rule at the source's window_len); a slot whose
 * destination page is unmapped is dropped, one whose source page is unmapped copies page 0's row.  Pages are copied,
 * never shared.  Skipped pairs and the aliasing rules are those of sfa_ring_copy_slots.  sfa_last_path():
 * "ring_copy_slots_paged".
 * FP8 pages: the eight buffers may all be SFA_DTYPE_FP8_E4M3 (a paged FP8 pool, below), as in sfa_ring_copy_slots: a
 * byte copy through both tables, 16 codes per piece, no scales - the caller keeps EQUAL kv_scale on pools that exchange
 * slots.  Mixed FP8 / 16-bit buffers are refused with the one-dtype text of sfa_ring_copy_slots.
 */
int sfa_ring_copy_paged_slots(const sfa_tensor* src_sink_k, const sfa_tensor* src_sink_v, const sfa_tensor* src_window_k,
                              const sfa_tensor* src_window_v, const int32_t* src_state, const sfa_tensor* dst_sink_k,
                              const sfa_tensor* dst_sink_v, const sfa_tensor* dst_window_k, const sfa_tensor* dst_window_v,
                              int32_t* dst_state, const int32_t* src_slots, const int32_t* dst_slots, int n_pairs,
                              const int32_t* src_page_table, int src_table_stride, const int32_t* dst_page_table,
                              int dst_table_stride, void* stream);

/*
 * Sharing pages on a fork (copy on first write).  Within ONE paged pool a fork need not copy the ring: the caller writes
 * the source's table row into the destination's row (host bookkeeping with reference counts, outside this library) and
 * calls sfa_ring_share_paged_slots for what is not paged.  Every later read of the destination goes through its own row
 * to the shared pages.  Before a storing call reaches a page that more than one row names, the caller gives the storing
 * slot a page of its own: a fresh entry in its row, then sfa_pages_copy(old page -> new page) on the same stream in front
 * of the storing call, once for every layer that reads the table.  A page that two rows name is therefore never stored
 * into.
 *
 * sfa_ring_share_paged_slots: the unpaged half of sfa_ring_copy_paged_slots.  For every live pair the live sink rows
 * (j < clamp(sink_len, 0, num_sink), all KV heads) and the state row (4 ints, verbatim) of slot src_slots[i] are copied
 * into slot dst_slots[i]; no ring memory is read or written and the call takes no ring buffers and no table.  Sinks and
 * state rows end bitwise as sfa_ring_copy_paged_slots leaves them for the same pairs.  Skipped pairs (-1 / out of range
 * on either side, s == d where src_state == dst_state) and the aliasing rules are those of sfa_ring_copy_slots.  One
 * launch on `stream`, capturable, nothing read on the host.  The sink buffers are bf16, f16, f32 or SFA_DTYPE_FP8_E4M3
 * (a byte copy, no scales).
 * Host checks, in this order: null descriptors ("src_sink_k: null tensor descriptor", ...); null src_state / dst_state /
 * src_slots / dst_slots; n_pairs < 0 (n_pairs == 0 returns SFA_OK without a launch); "ring_share_slots: <name> and
 * src_sink_k differ in dtype (the four buffers must share one)"; equal Hkv, num_sink, D ("ring_share_slots: <name> must
 * be [S, H_kv, num_sink, D] = ..."); one shape[0] >= 1 within each pool; rows a multiple of 16 bytes and 16-byte aligned.
 * sfa_last_path(): "ring_share_slots_paged".
 */
int sfa_ring_share_paged_slots(const sfa_tensor* src_sink_k, const sfa_tensor* src_sink_v, const int32_t* src_state,
                               const sfa_tensor* dst_sink_k, const sfa_tensor* dst_sink_v, int32_t* dst_state,
                               const int32_t* src_slots, const int32_t* dst_slots, int n_pairs, void* stream);

/*
 * sfa_pages_copy: copy whole ring pages within the page buffers of one layer.  window_k / window_v [n_pages, Hkv, P, D]
 * are bf16, f16 or SFA_DTYPE_FP8_E4M3, both of one dtype and shape; src_pages / dst_pages are device int32 [n_pairs].
 * Pair i copies page src_pages[i] onto page dst_pages[i], K and V, every head and row, as bytes (no scales).
 *   - Skipped pairs, decided on the device: either entry outside [0, n_pages) (compared as unsigned, so -1 is outside),
 *     or both entries equal.
 *   - Undefined, and not validated: one destination named twice; a destination that is also a source of the same call.
 * One launch on `stream`, capturable, no workspace, nothing read on the host.  A workgroup reads its pair's two page ids
 * once; each thread moves 16-byte pieces and holds several of K and of V in flight before its first store; the grid is
 * n_pairs x the pieces of a page.  Page, head and row offsets are 64-bit products of the descriptor's strides: the
 * buffers may be strided views and a page buffer may exceed 4 GiB.
 * Host checks, in this order, SFA_ERR_INVALID_ARGUMENT: null descriptors ("window_k: null tensor descriptor"); n_pairs
 * < 0; unequal shapes or dtypes ("window_k and window_v differ in shape[i]: ...", "... differ in dtype"); "pages_copy:
 * the page buffers hold bf16, f16 or FP8 (e4m3) (got dtype d)"; "pages_copy: the page buffers need shape[0] = n_pages in
 * [1, 2^30) (got n)"; n_pairs == 0 returns SFA_OK here, without a launch; "src_pages: null device pointer" /
 * "dst_pages: ..."; "pages_copy: K/V rows must be a multiple of 16 bytes (head dim n)"; "pages_copy: rows of every tensor
 * must be 16-byte aligned".  sfa_last_path(): "pages_copy".
 */
int sfa_pages_copy(const sfa_tensor* window_k, const sfa_tensor* window_v, const int32_t* src_pages,
                   const int32_t* dst_pages, int n_pairs, void* stream);

/*
 * Paged FP8 slot pool: the two pools above composed - the ring memory follows the sequence length AND holds one byte per
 * element.  Nothing new is defined here; each rule is the one of the pool it comes from:
 *   window_k/v  [n_pages, Hkv, P, D] SFA_DTYPE_FP8_E4M3: the ring pages hold e4m3fn codes.  P, page_table, table_stride,
 *               Wc = table_stride * P, unmapped entries (a read goes to page 0, a store is dropped, the state row still
 *               advances), the prefix rule and 64-bit page and row addresses are those of the paged pool.  A page is
 *               Hkv * P * D BYTES: every page and row offset is taken at one byte per element.
 *   sink_k/v    [S, Hkv, num_sink, D] SFA_DTYPE_FP8_E4M3, not paged.
 *   kv_scale    device float [2][Hkv] or null, with the storing rule, the clamp and the reading rule of the FP8 pool.
 *   q / k_new / v_new / o (k / v of the fill) are bf16 or f16, head dims 64 / 80 / 96 / 128.
 * Contract, bitwise (pages8 = the page buffers, table, scale as above):
 *   - Read vs the contiguous FP8 twin.  o equals o of the same call of the *_fp8_slots family on the contiguous FP8
 *     pool window[s, :, j P : (j + 1) P] = pages8[table[s][j]] with the same sinks, state and scales.
 *   - Read vs the 16-bit paged pool.  o equals o of the same *_paged_slots call on a 16-bit pool with the same table
 *     whose pages and sinks hold T(float(code) * scale).
 *   - Storage.  After a storing call every mapped page row holds the storing rule applied to the row the same call
 *     writes into a 16-bit paged pool with the same table; every other byte of the page buffers keeps its value; stores
 *     to unmapped pages are dropped; the sinks hold what the *_fp8_slots sibling stores; the state rows are equal.
 *   - Copy.  After sfa_ring_copy_paged_slots every later call on the destination is bitwise the call on the source,
 *     within a pool and between two pools of equal scales, geometry and P.
 * Host checks, in this order: those the paged pool adds (above, with <call> as below); then those of the *_fp8_slots
 * sibling in their order, "<call>: the cache buffers must be FP8 (e4m3)" where the dtypes are compared (a 16-bit page
 * buffer ends here); then SFA_ERR_UNSUPPORTED for fp32 activations, other head dims or SFA_FLAG_FORCE_GENERIC: "<call>:
 * a paged FP8 pool serves bf16 / f16 activations at head dims 64 / 80 / 96 / 128 (got dtype d, head dim n[,
 * SFA_FLAG_FORCE_GENERIC])".  <call> is decode_ragged_paged_fp8, ring_commit_ragged_paged_fp8 or
 * ring_fill_varlen_paged_fp8.
 *
 * sfa_decode_ring_ragged_paged_fp8_slots: the arguments of sfa_decode_ring_ragged_paged_slots plus kv_scale in front of
 * workspace.  Workspace: sfa_decode_ragged_workspace_bytes with q's dtype and Nkv_cache = num_sink + table_stride * P.
 * sfa_last_path(): the name of the 16-bit contiguous call plus "_paged_kvfp8".
 */
int sfa_decode_ring_ragged_paged_fp8_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                           const sfa_tensor* window_k, const sfa_tensor* window_v,
                                           const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                                           const float* s_aux, const int32_t* parent, const int32_t* commit_seq,
                                           int commit, int32_t* state, const int32_t* slots, const int32_t* cu_q,
                                           int n_seq, const int32_t* page_table, int table_stride,
                                           const float* kv_scale, void* workspace, size_t workspace_bytes, float scale,
                                           unsigned flags, void* stream);

/* sfa_ring_commit_path_ragged_paged_slots into FP8 pages: the same arguments plus kv_scale in front of stream; each row
 * is quantised as it is stored through the table.  sfa_last_path(): "ring_commit_path_ragged_slots_paged_kvfp8". */
int sfa_ring_commit_path_ragged_paged_fp8_slots(const sfa_tensor* window_k, const sfa_tensor* window_v,
                                                const sfa_tensor* k_new, const sfa_tensor* v_new, const int32_t* count,
                                                const int32_t* path, const int32_t* cu_q, int n_seq, int32_t* state,
                                                const int32_t* slots, const int32_t* page_table, int table_stride,
                                                int n_slots, const float* kv_scale, void* stream);

/* sfa_ring_fill_varlen_paged_slots into a paged FP8 pool: the same arguments plus kv_scale in front of stream.
 * sfa_last_path(): "ring_fill_varlen_slots_paged_kvfp8". */
int sfa_ring_fill_varlen_paged_fp8_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                         const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v,
                                         const int32_t* cu_seqlens, int n_seq, int32_t* state, const int32_t* slots,
                                         const int32_t* page_table, int table_stride, const float* kv_scale,
                                         void* stream);

/* ---- Export: the inverse of sfa_ring_fill_varlen_slots.
 *
 * sfa_ring_export_slots writes the live tokens of n_seq named slots of a pool, in TOKEN order, into a pack of the layout
 * the fills take - what hands a request to another process or device, moves it into a pool of another shape (a longer
 * ring, another page size, 16-bit <-> FP8: export here, sfa_ring_fill_varlen_*_slots there), or spills it to the host.
 *   sink_k/v [S, Hkv, num_sink, D]   window_k/v [S, Hkv, Wc, D]   state int32 [S][4] (const: read only)
 *   k_out, v_out [1, Hkv, T, D]      cu_seqlens device int32 [n_seq + 1]   slots device int32 [n_seq]
 *   pos_out      device int32 [T] or NULL
 * Sequence i owns the packed rows [cu[i], cu[i + 1]) (m_i of them; offsets read on the device, clamped into [0, T] and
 * made non-decreasing as sfa_ring_fill_varlen does) and names slot c = slots[i].  Its state row {sl = sink_len, wl =
 * window_len, wp = write_pos, seen} is clamped as the attention kernels clamp it (sl into [0, num_sink], wl into [0, Wc],
 * wp into [0, Wc - 1]); live = sl + wl tokens are held, and token-order index j is
 *   - j < sl: sink row j, at position j;
 *   - j = sl + r, r < wl: ring slot (wp - wl + r) mod Wc, at position seen - wl + r - the oldest ring token first.  That is
 *     slot r while the ring fills (every placement above keeps wp == wl until the ring is full) and after a prefill
 *     (sfa_ring_fill_varlen leaves a full ring at wp == 0 with the oldest token in slot 0), and slot (wp + r) mod Wc once
 *     commits have wrapped a full ring (a commit stores token t at (wp + t) mod Wc and advances wp, so the oldest live
 *     token sits at the new wp).
 * Row j < min(m_i, live) of the sequence receives token j, all KV heads.  EVERY other row of the pack is written as
 * zeros, so a pack exported at a fixed T is fully defined: rows j >= live of a sequence (m_i > live), the rows of a
 * sequence whose slot is outside [0, S) (the slots = -1 rule), and rows that no sequence covers (in front of cu[0], behind
 * cu[n_seq]).  m_i < live truncates: the first m_i tokens are written.  pos_out[row] = the token's position, -1 on a
 * zeroed row.  A sequence of a fresh slot (all-zero state row) has live = 0.
 *   - The pack has the pool's dtype (bf16, f16 or f32) and the rows are copied verbatim, 16 bytes per thread and buffer.
 *   - Nothing of the pool, the state or the table is written; nothing is read on the host.  One launch on `stream`, no
 *     workspace, no allocation, no atomics: capturable, and a repeated call is bitwise identical.  The same slot may be
 *     named twice.  The grid follows T (Hkv * T rows), not the pool's capacity; every offset is formed in 64 bits from the
 *     descriptors' strides, as in the packed calls (a pack behind a 4 GiB head stride, a slot past 4 GiB).
 *   - Undefined: a pool buffer that overlaps k_out / v_out / pos_out (not checked).
 * Host checks before anything launches, SFA_ERR_INVALID_ARGUMENT: null descriptors; unequal shapes within (sink_k,
 * sink_v), (window_k, window_v), (k_out, v_out); null cu_seqlens / state / slots; n_seq >= 1; "packed layout: k_out /
 * v_out must be [1, H_kv, T, D] (batch dim n)"; "k_out / v_out and the cache buffers must share one dtype"; one S >= 1;
 * the pool's Hkv and D; rows a multiple of 16 bytes and 16-byte aligned ("ring_export: rows of every tensor must be
 * 16-byte aligned").  T == 0 returns SFA_OK without a launch.  sfa_last_path(): "ring_export_slots".
 *
 * sfa_ring_export_fp8_slots: an FP8 pool; the same arguments plus kv_scale (device float [2][Hkv] or NULL = ones) in
 * front of stream.  k_out / v_out are bf16 or f16 (T) and every element is T(float(code) * scale[h]), the reading rule
 * above through the same device function as the packed step: bit for bit what that step feeds its LDS.  A thread reads
 * 8 codes and writes 16 bytes.  "ring_export_fp8: the cache buffers must be FP8 (e4m3)"; fp32 packs and head dims outside
 * 64 / 80 / 96 / 128 are SFA_ERR_UNSUPPORTED.  sfa_last_path(): "ring_export_slots_kvfp8".
 *
 * sfa_ring_export_paged_slots: a paged pool (window_k/v = the pages); the same arguments plus (page_table, table_stride)
 * in front of stream, checked as the paged pool documents under the name ring_export_paged.  A ring slot is read from row
 * slot mod P of its page; a slot whose table entry is unmapped reads nothing: its row is zeros and pos_out still gives
 * its position.  sfa_last_path(): "ring_export_slots_paged".
 *
 * sfa_ring_export_paged_fp8_slots: both, (page_table, table_stride, kv_scale) in front of stream, byte offsets at one
 * byte per element.  sfa_last_path(): "ring_export_slots_paged_kvfp8".
 */
int sfa_ring_export_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                          const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out,
                          const int32_t* cu_seqlens, int n_seq, const int32_t* state, const int32_t* slots,
                          int32_t* pos_out, void* stream);

int sfa_ring_export_fp8_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                              const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out,
                              const int32_t* cu_seqlens, int n_seq, const int32_t* state, const int32_t* slots,
                              int32_t* pos_out, const float* kv_scale, void* stream);

int sfa_ring_export_paged_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out,
                                const int32_t* cu_seqlens, int n_seq, const int32_t* state, const int32_t* slots,
                                int32_t* pos_out, const int32_t* page_table, int table_stride, void* stream);

int sfa_ring_export_paged_fp8_slots(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                                    const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out,
                                    const int32_t* cu_seqlens, int n_seq, const int32_t* state, const int32_t* slots,
                                    int32_t* pos_out, const int32_t* page_table, int table_stride,
                                    const float* kv_scale, void* stream);

/* ---- Fork groups: a shared prompt prefix is read once per group.
 *
 * sfa_decode_ring_ragged_group_paged_slots / sfa_decode_ring_ragged_group_paged_fp8_slots: the arguments of their paged
 * siblings without `parent`, plus (cu_g, n_grp) behind (cu_q, n_seq).  cu_g: device int32 [n_grp + 1], offsets over the
 * SEQUENCES of the pack, clamped into [0, n_seq] and made non-decreasing pairwise as cu_q is; group g is the consecutive
 * sequences [cu_g[g], cu_g[g + 1]); a sequence that no group covers is ungrouped.  Never read on the host.
 *
 * The caller promises nothing about the groups: a preparation launch reads the state rows and the table and decides per
 * group a shared length Lg, the largest multiple of P such that every MEMBER (an active sequence with n_i > 0; inactive
 * and empty ones are skipped)
 *   - is not admitting (SFA_FLAG_RAGGED_ADMIT and a fresh slot),
 *   - has window_len + n_i <= Wc and write_pos == window_len (the ring is unwrapped and stays so within the step),
 *   - has Lg <= window_len,
 *   - has table entries j < Lg / P that are mapped and equal those of the group's first member.
 * A group with fewer than two members has Lg = 0.  Groups must not overlap: if cu_g, clamped, decreases anywhere, every
 * group of the call has Lg = 0 (the pairwise clamp alone would let [0, 4, 2, 6] name sequences 2 and 3 twice), so o is
 * defined - the ungrouped call's - for any cu_g.  Ring slots [0, Lg) are then read once per 32-row block of the group's
 * packed rows (from the first member's pages); every member reads its sinks, its ring slots [Lg, window_len) and its
 * chunk itself.
 *   - o is the softmax over exactly the keys the ungrouped call sees, within the tolerance of that call; where every
 *     group has Lg = 0 it is bitwise the ungrouped call's.  The partition of a row's keys into splits depends on Lg, on the
 *     call's shape and on the sequence's own (state row, n_i) only, and the fold order is fixed (the row's own partials,
 *     its group's, s_aux): the same inputs give the same bits, under any grouping that yields the same Lg.
 *   - Commit, advance, commit_seq, zeros for inactive and empty rows and the state-ordering rule are those of
 *     sfa_decode_ring_ragged_paged_slots: the pool and the state rows end bitwise as the ungrouped call leaves them.  The
 *     preparation launch only reads state rows and table; the advance stays the call's last launch.
 * Workspace: sfa_decode_ragged_group_workspace_bytes(n_seq, n_grp, Hq, Hkv, T, Nkv_cache = num_sink + table_stride * P, D,
 * dtype): the ungrouped workspace plus the group partials and tables; 0 for shapes no grouped instance serves (fp32, head
 * dims other than 64 / 80 / 96 / 128).  Host checks: those of the sibling in its order, with "cu_g: null device pointer"
 * and "decode_ragged: n_grp (n) must be at least 1" behind the n_seq check.  sfa_last_path(): the sibling's with "_group"
 * in front of the pool tag ("..._ragged_commit_group_paged").  Out of scope: draft trees inside a group (no parent
 * argument), groups on contiguous pools, a wrapped shared prefix, shared sink rows. */
size_t sfa_decode_ragged_group_workspace_bytes(int64_t n_seq, int64_t n_grp, int64_t Hq, int64_t Hkv, int64_t T,
                                               int64_t Nkv_cache, int64_t D, int dtype);

int sfa_decode_ring_ragged_group_paged_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                             const sfa_tensor* window_k, const sfa_tensor* window_v,
                                             const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                                             const float* s_aux, const int32_t* commit_seq, int commit, int32_t* state,
                                             const int32_t* slots, const int32_t* cu_q, int n_seq, const int32_t* cu_g,
                                             int n_grp, const int32_t* page_table, int table_stride, void* workspace,
                                             size_t workspace_bytes, float scale, unsigned flags, void* stream);

int sfa_decode_ring_ragged_group_paged_fp8_slots(const sfa_tensor* q, const sfa_tensor* sink_k, const sfa_tensor* sink_v,
                                                 const sfa_tensor* window_k, const sfa_tensor* window_v,
                                                 const sfa_tensor* k_new, const sfa_tensor* v_new, const sfa_tensor* o,
                                                 const float* s_aux, const int32_t* commit_seq, int commit,
                                                 int32_t* state, const int32_t* slots, const int32_t* cu_q, int n_seq,
                                                 const int32_t* cu_g, int n_grp, const int32_t* page_table,
                                                 int table_stride, const float* kv_scale, void* workspace,
                                                 size_t workspace_bytes, float scale, unsigned flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFA_H */
