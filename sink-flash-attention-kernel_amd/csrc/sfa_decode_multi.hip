// Multi-token decode over the sink + ring KV cache (speculative verify, chunked continuation): n new queries attend to
// the cache as it is BEFORE the chunk plus the chunk itself, with the mask n successive single-token steps would apply.
//
// Key positions.  Every key gets a chronological position c relative to the chunk start: sink rows are always visible;
// ring slot s (0 <= s < window_len) holds the token of position c = ((s - write_pos + window_len) mod Wc) - window_len
// (-window_len = oldest, -1 = newest); chunk token u has c = u.  Query t sees c in [t - Wc + 1, t].  Softmax is order-free,
// so the ring is walked in PHYSICAL slot order (contiguous rows); c is only needed for the mask.
//
// MFMA path (bf16 / f16, head dims 64 / 80 / 96 / 128): the G = H_q / H_kv query heads and the n chunk queries of one
// KV head are R = G * n rows, ordered rho = t * G + g, cut into 32-row blocks (a block covers ceil(32 / G) consecutive
// queries, so its mask band is narrow).  A workgroup = (batch, KV head, key split, row block), 4 waves; the split's
// 32-key tiles are dealt round-robin to the waves, each wave streams its tiles through its own LDS slot (no barriers in
// the loop) with the next tile's global loads in flight during the current tile's math:
//   * X^T = K Q^T with mfma_f32_32x32x16 (keys on the accumulator rows, the block's query rows on the lanes): the
//     per-row max / sum are per-lane values plus one half-wave swap;
//   * O^T += V^T X^T takes the (exponentiated) accumulator as the B operand without lane movement, V^T comes from LDS
//     by ds_read_b64_tr_b16 - the layouts of the forward kernel (sfa_fwd_mfma.hip);
//   * every tile is classified scalar-wise against the block's [t_min, t_max]: full (no mask work), edge (per-element
//     mask) or dead (skipped, never loaded).
// At the end of the split the 4 waves merge (m, l, O) through LDS in a fixed order and write one partial per row.
// The f32-accumulate path (fp32, other head dims up to 1 KiB per row) writes the same partials, one wave per row.
// The reduce kernel folds the partials and the s_aux virtual split (m = s_aux, l = 1, o = 0) in split order and writes
// o in q's dtype; with `commit` its trailing workgroups then store the chunk into the ring (stream order puts that
// after every read of the slots it overwrites; the split kernels never write the cache).  No atomics anywhere: the same
// inputs give bitwise-identical outputs.
#include "sfa_common.hpp"
#include "sfa_internal.hpp"

#include <climits>
#include <type_traits>

namespace sfa {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    using frag = bf16x8_t;
    using elem = __bf16;
    static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma<f16_t> {
    using frag = f16x8_t;
    using elem = _Float16;
    static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};

// ---- FP8 pool (the *_fp8_slots calls).  The cache buffers hold OCP e4m3fn codes, one byte per element;
// the activations stay 16-bit.  A third kernel argument that only the FP8 instances take (`KA...` / the tail of `RA...`
// is empty for every other instance, as with RaggedArgs): scale = device float [2][Hkv], row 0 K and row 1 V, null = ones.
struct Kv8Args {
    const float* scale;
};

// the scale of KV head hk: row 0 for K, 1 for V
__device__ __forceinline__ float kv8_scale(const Kv8Args& kv, int row, int Hkv, int hk) {
    return kv.scale ? kv.scale[row * Hkv + hk] : 1.f;
}

// reading: the 8 codes of one 8-byte piece -> 8 elements of T, each T(float(code) * s): one f32 multiply, then the
// round-to-nearest-even conversion.  Byte i of the piece is element i.
// Pairs (the export, whose output is compared bit by bit): the products are converted two at a time by the packed
// conversion.  Converted one by one, the compiler fuses some lanes' multiply and f16 conversion into one instruction that
// adds +0, which turns the code of -0 into +0 there - invisible to an attention product, visible in exported bytes.
template <typename T, bool Pairs = false>
__device__ __forceinline__ u32x4 kv8_read(unsigned lo, unsigned hi, float s) {
    using E = typename Mma<T>::elem;
    typename Mma<T>::frag out;
    const unsigned w[2] = {lo, hi};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
        const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        if constexpr (Pairs) {
            typedef E e2 __attribute__((ext_vector_type(2)));
            const e2 ca = __builtin_convertvector(a * s, e2), cb = __builtin_convertvector(b * s, e2);
            out[4 * i + 0] = ca[0], out[4 * i + 1] = ca[1], out[4 * i + 2] = cb[0], out[4 * i + 3] = cb[1];
            continue;
        }
        out[4 * i + 0] = (E)(a[0] * s);
        out[4 * i + 1] = (E)(a[1] * s);
        out[4 * i + 2] = (E)(b[0] * s);
        out[4 * i + 3] = (E)(b[1] * s);
    }
    return __builtin_bit_cast(u32x4, out);
}

// storing: 8 elements of the 16-bit type Q (16 bytes) -> 8 codes, each e4m3fn_rne(clamp(float(x) * r, -448, 448)) with
// r = 1.0f / scale (the caller's division).  The clamp is explicit: the conversion never sees a value it would overflow on.
template <typename Q>
__device__ __forceinline__ uint2 kv8_quant(u32x4 raw, float r) {
    const typename Mma<Q>::frag e = __builtin_bit_cast(typename Mma<Q>::frag, raw);
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = fminf(fmaxf((float)e[i] * r, -448.f), 448.f);
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    return make_uint2((unsigned)lo, (unsigned)hi);
}

// one piece (8 elements of K and of V, KV head hk) of a storing kernel.  Q = void: source and destination share the
// dtype, 16 bytes are copied.  Q = the 16-bit source type of an FP8 pool: 16 bytes read, quantised, 8 bytes written.
template <typename Q>
__device__ __forceinline__ void store_piece(char* kd, char* vd, const char* ks, const char* vs,
                                            [[maybe_unused]] const Kv8Args& kv, [[maybe_unused]] int Hkv,
                                            [[maybe_unused]] int hk) {
    if constexpr (std::is_void_v<Q>) {
        *reinterpret_cast<u32x4*>(kd) = *reinterpret_cast<const u32x4*>(ks);
        *reinterpret_cast<u32x4*>(vd) = *reinterpret_cast<const u32x4*>(vs);
    } else {
        const u32x4 kr = *reinterpret_cast<const u32x4*>(ks), vr = *reinterpret_cast<const u32x4*>(vs);
        *reinterpret_cast<uint2*>(kd) = kv8_quant<Q>(kr, 1.0f / kv8_scale(kv, 0, Hkv, hk));
        *reinterpret_cast<uint2*>(vd) = kv8_quant<Q>(vr, 1.0f / kv8_scale(kv, 1, Hkv, hk));
    }
}
// bytes per element of the destination and byte offset of piece ch in a destination row
template <typename Q> __device__ __forceinline__ int piece_es(int es) { return std::is_void_v<Q> ? es : 1; }
template <typename Q> __device__ __forceinline__ int64_t piece_off(int ch) { return (int64_t)ch * (std::is_void_v<Q> ? 16 : 8); }

constexpr int kTile = 32;        // keys per tile
constexpr int kWaves = 4;        // waves per workgroup of the MFMA split kernel
constexpr int kMinTiles = 4;     // a split gives every wave at least one tile

struct MultiArgs {
    View q, sk, sv, wk, wv, kn, vn, o;
    const float* s_aux;
    float *Mp, *Lp, *Op;         // partials [rows][Sw], [rows][Sw], [rows][Sw][D]; rows = B * Hkv * R
    int B, Hkv, G, n, D, R, nrb;
    int sink_len, wl, wp, wc;    // cache state before the chunk; wc = ring capacity
    int T0, T1, T;               // tiles: sink [0, T0), ring [T0, T1), chunk [T1, T)
    int tps, S;                  // tiles per split, splits
    int Sw;                      // launched splits = stride of the partials (S, or the full-cache bound in dyn mode)
    float scale_log2;            // softmax scale * log2(e): scores live in the log2 domain up to the output
    int commit;
    // dyn mode (sfa_decode_ring_multi_dyn): state = device {sink_len, window_len, write_pos}; every workgroup reads it and
    // replans (T0, T1, T, tps, S) with multi_plan.  Null: the host plan above holds.
    const int* state;
    int sstride;                 // state row stride: 0 = one state shared by the batch, 4 = per-sequence rows [B][4]
    int ns;                      // sink buffer rows (dyn: clamp of sink_len)
    int want;                    // want_splits(B, Hkv, nrb): the workgroup-target cap of the split count
    // tree calls (sfa_decode_ring_tree*): parent[b * pstride + u], u < n <= 64 (pstride 0: one tree shared by the batch)
    const int* parent;
    int pstride;
    // path commit (sfa_ring_commit_path_*): chunk token path[b * pathstride + j] is the j-th one stored
    const int* path;
    int pathstride;
    // slot calls (sfa_*_slots): batch row b works on cache row and state row slots[b] of a pool of npool rows; a value
    // outside [0, npool) marks an inactive row.  Null: cache row b (every other call).
    const int* slots;
    int npool;
};

// packed calls (sfa_decode_ring_ragged_slots): a second kernel argument that only the ragged instances take.  q / k_new
// / v_new / o are [1, H, T, D] packs; sequence i = packed rows [cu_q[i], cu_q[i + 1]) (offsets clamped into [0, T] and
// made non-decreasing, as ring_fill_varlen_kernel does) works on cache row slots[i].  In MultiArgs B = 1, n / R are
// set per workgroup (wave) from cu_q, nrb = the row-block bound ceil(G * T / 32) + n_seq, partial rows are indexed by
// packed row: (hk * T + packed row) * G + g.
struct RaggedArgs {
    const int* cu_q;             // [n_seq + 1], device, not validated
    const int2* blk;             // [nrb] row-block id -> (sequence, local 32-row block); sequence -1: surplus
    const int* rowseq;           // [T] packed row -> sequence, -1: covered by none (padding)
    int n_seq, T;
    int admit;                   // SFA_FLAG_RAGGED_ADMIT: a sequence on a fresh slot (state row seen == 0) is admitted
    // per-sequence commit: with `commit`, sequence i is stored and advanced iff commit_seq[i] != 0 (null: every
    // sequence).  Read by commit_piece_ragged and ring_advance_ragged_kernel only.
    const int* commit_seq;       // [n_seq], device, or null
};

// ---- paged pool (the *_paged_slots calls).  The ring buffers are PAGES [n_pages, Hkv, P, D] (the
// page index where the slot index was, same strides); table[c * stride + j] is the page that holds ring slots
// [j P, (j + 1) P) of cache row c.  P = 1 << shift >= kTile, Wc = stride * P, so a 32-slot ring tile lies inside one page.
// A kernel argument that only the paged instances take, like Kv8Args.  A pool that is FP8 AND paged
// takes both, Kv8Args first: its pages hold codes, and every page and row offset is in bytes of ONE per element.
struct PageArgs {
    const int* table;            // device int32 [S][stride]; read when the kernel runs, never on the host
    int stride;
    int shift;
    int npages;
};

// ---- fork groups (the *_group_paged_slots calls).  Group g = the consecutive sequences
// [cu_g[g], cu_g[g + 1]) of the pack.  group_prep_kernel decides a shared length Lg per group (ring slots [0, Lg) are the
// same pages for every member, unwrapped and visible to every row); those slots are read once per 32-row block of the
// GROUP's rows by the shared-phase workgroups (the first `nsh` block ids of the split launch), which write one partial per
// row and group split into the second partial area (Mg, Lg, Og; stride Sgw).  A member's own workgroups skip [0, Lg).
// The last trailing argument, and the `Grouped` flag of an instance: an instance is grouped iff its pack ends in GroupArgs
// (has_arg below) - the flag is read off the pack and is no template parameter, so that every instance without groups
// keeps its name.
struct GroupArgs {
    const int* cu_g;             // [n_grp + 1], device, not validated: offsets over the sequences of the pack
    int n_grp;
    const int2* gblk;            // [ngrb] group row-block id -> (group, local 32-row block); group -1: surplus
    const int2* glg;             // [n_grp] (Lg, cache row of the group's first active non-empty member)
    const int* gseq;             // [n_seq] sequence -> its group, -1: ungrouped
    float *Mg, *Lg, *Og;         // the group partials [rows][Sgw], [rows][Sgw], [rows][Sgw][D], rows as in MultiArgs
    int ngrb;                    // the group row-block bound ceil(G * T / 32) + n_grp
    int Sgw;                     // launched group splits = stride of the group partials: the bound over Lg <= Wc
    int want_g;                  // want_splits(1, Hkv, ngrb): the cap of a group's split count
    int nsh;                     // shared-phase block ids of the split launch: Hkv * Sgw * ngrb rounded up to 8
};

// The optional trailing arguments of a kernel (`RA...` behind MultiArgs, `KA...` behind a storing kernel's own): of
// RaggedArgs, Kv8Args, PageArgs and GroupArgs, in that order, an instance takes the ones its flags name and no other - its
// signature, argument block and code stay those of a kernel without the others.  arg_of<W>(pack...) is the member of
// type W by reference, or a W of zeros where the instance takes none (Kv8Args: scale null = all ones).
template <typename W>
__device__ __forceinline__ W arg_of() { return W{}; }
template <typename W, typename A0, typename... A>
__device__ __forceinline__ decltype(auto) arg_of(const A0& a0, const A&... rest) {
    if constexpr (std::is_same_v<W, A0>) return (a0);
    else return arg_of<W>(rest...);
}
template <typename W, typename... A>
constexpr bool has_arg = (std::is_same_v<A, W> || ...);
// the guard of every kernel with such a pack: exactly the arguments that the flags name (their order is dispatch_pool's);
// GroupArgs may follow on a (Ragged, Paged) instance
template <bool Ragged, bool KV8, bool Paged, typename... A>
constexpr bool tail_is = sizeof...(A) == (Ragged ? 1 : 0) + (KV8 ? 1 : 0) + (Paged ? 1 : 0) + (has_arg<GroupArgs, A...> ? 1 : 0) &&
                         has_arg<RaggedArgs, A...> == Ragged && has_arg<Kv8Args, A...> == KV8 &&
                         has_arg<PageArgs, A...> == Paged && !(has_arg<GroupArgs, A...> && !(Ragged && Paged));

// the page of ring slot `slot` (in [0, Wc)) of cache row c; -1: the entry is unmapped ((unsigned)e >= n_pages).  A read
// of an unmapped page addresses page 0, a store to one is dropped.  The index is 64-bit; slot >> shift < stride.
__device__ __forceinline__ int page_at(const PageArgs& pg, int c, int slot) {
    const int e = pg.table[(int64_t)c * pg.stride + (slot >> pg.shift)];
    return (unsigned)e < (unsigned)pg.npages ? e : -1;
}
__device__ __forceinline__ int page_row(const PageArgs& pg, int slot) { return slot & ((1 << pg.shift) - 1); }

// sequence i of the pack: first packed row and length
struct RaggedSeq {
    int c0, n;
};

__device__ __forceinline__ RaggedSeq ragged_seq(const RaggedArgs& rg, int i) {
    int c0 = rg.cu_q[i], c1 = rg.cu_q[i + 1];
    c0 = c0 < 0 ? 0 : (c0 > rg.T ? rg.T : c0);
    c1 = c1 < c0 ? c0 : (c1 > rg.T ? rg.T : c1);
    return RaggedSeq{c0, c1 - c0};
}

// the preparation launch of a packed call: one workgroup writes the two tables from cu_q alone (it reads no cache state,
// so the state-ordering rule is unaffected).  Sequence i owns the block ids [start_i, start_i + ceil(G n_i / 32)) with
// start_i = floor(G c0_i / 32) + i: no scan is needed, the ranges are disjoint (floor(x + y) + 1 >= floor(x) + ceil(y))
// and end below ceil(G T / 32) + n_seq; start_i and c0_i increase with i, so both maps are a binary search for the
// last sequence that starts at or before the id, followed by a range check (offsets that are not monotonic find some
// sequence or none, never an index outside the pack).
__global__ __launch_bounds__(1024) void ragged_prep_kernel(RaggedArgs rg, int2* blk, int* rowseq, int G, int nrb) {
    for (int x = threadIdx.x; x < nrb + rg.T; x += 1024) {
        const bool row = x >= nrb;
        const int id = row ? x - nrb : x;
        int lo = 0, hi = rg.n_seq - 1;       // the last i with start(i) <= id; sequence 0 starts at 0
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            const int c = ragged_seq(rg, mid).c0;
            const int64_t start = row ? c : (int64_t)G * c / 32 + mid;
            if (start <= id) lo = mid;
            else hi = mid - 1;
        }
        const RaggedSeq s = ragged_seq(rg, lo);
        if (row) {
            rowseq[id] = (id >= s.c0 && id < s.c0 + s.n) ? lo : -1;
        } else {
            const int64_t local = id - ((int64_t)G * s.c0 / 32 + lo);
            const bool hit = local >= 0 && local * 32 < (int64_t)G * s.n;
            blk[id] = hit ? make_int2(lo, (int)local) : make_int2(-1, 0);
        }
    }
}

// group g of the pack: its sequences [i0, i1) (cu_g clamped into [0, n_seq] and made non-decreasing pairwise, as
// ragged_seq does for cu_q) and its packed rows [c0, c0 + n): from the first row of sequence i0 to the end of sequence
// i1 - 1.  An empty group has n = 0.
struct GroupSpan {
    int i0, i1, c0, n;
};

__device__ __forceinline__ GroupSpan group_span(const RaggedArgs& rg, const GroupArgs& gr, int g) {
    int i0 = gr.cu_g[g], i1 = gr.cu_g[g + 1];
    i0 = i0 < 0 ? 0 : (i0 > rg.n_seq ? rg.n_seq : i0);
    i1 = i1 < i0 ? i0 : (i1 > rg.n_seq ? rg.n_seq : i1);
    if (i1 == i0) return GroupSpan{i0, i1, 0, 0};
    const RaggedSeq a = ragged_seq(rg, i0), z = ragged_seq(rg, i1 - 1);
    const int n = z.c0 + z.n - a.c0;
    return GroupSpan{i0, i1, a.c0, n < 0 ? 0 : n};
}

inline __host__ __device__ int cdiv_i(int x, int y) { return (x + y - 1) / y; }

struct MultiPlan {
    int T0, T1, T, tps, S;
};

// the tile / split plan of one cache state; the host (sfa_decode_ring_multi) and the dyn kernels (from the device state)
// both call it, so that the same state gives the same tile-to-split assignment bitwise.  Every count < 2^30.
inline __host__ __device__ MultiPlan multi_plan(int sink_len, int wl, int n, int want) {
    MultiPlan p;
    p.T0 = cdiv_i(sink_len, kTile);
    p.T1 = p.T0 + cdiv_i(wl, kTile);
    p.T = p.T1 + cdiv_i(n, kTile);
    // max_splits(Nkv = sink_len + wl + n), then at most one split per kMinTiles tiles
    int s = cdiv_i(cdiv_i(sink_len + wl + n, kTile) + 2, kMinTiles);
    if (s > want) s = want;
    if (s < 1) s = 1;
    const int s_tiles = cdiv_i(p.T, kMinTiles);
    if (s > s_tiles) s = s_tiles;
    p.tps = cdiv_i(p.T, s);
    p.S = cdiv_i(p.T, p.tps);
    return p;
}

// the state-dependent part of the arguments, kept apart from the (read-only, kernarg) MultiArgs
struct Fill {
    int sink_len, wl, wp;
    int T0, T1, T, tps, S;
    int nsk;                     // admitting sequence of a packed call: its first nsk chunk tokens are its sinks; else 0
};

// The prefill placement of SinkCacheLayer._prefill for a sequence of L tokens (ring_fill_varlen_kernel and the
// admitting sequences of a packed call): sink row j <- token j for j < sl = min(L, ns); with rem = L - sl, ring slot s <-
// token sl + s for s < rem when rem <= Wc, else token L - Wc + s (the newest Wc, wrapped at slot 0).
struct FillPlace {
    int L, ns, wc, sl, rem;
};

__device__ __forceinline__ FillPlace fill_place(int L, int ns, int wc) {
    const int sl = L < ns ? L : ns;
    return FillPlace{L, ns, wc, sl, L - sl};
}

// destination j of the (ns + Wc) rows of a cache row (j < ns: sink row j, else ring slot j - ns) -> the token stored
// there, -1: the row keeps its content
__device__ __forceinline__ int fill_src(const FillPlace& p, int j) {
    if (j < p.ns) return j < p.sl ? j : -1;
    const int s = j - p.ns;
    return p.rem <= p.wc ? (s < p.rem ? p.sl + s : -1) : p.L - p.wc + s;
}

// token t -> its destination j, -1: not stored.  The inverse of fill_src by construction: the only row that can hold t is
// tried and fill_src decides.
__device__ __forceinline__ int fill_dst(const FillPlace& p, int t) {
    const int j = t < p.sl ? t : p.ns + (p.rem <= p.wc ? t - p.sl : t - (p.L - p.wc));
    return (j >= 0 && j < p.ns + p.wc && fill_src(p, j) == t) ? j : -1;
}

// the state row {sink_len, window_len, write_pos, seen} after the placement (rem <= 0: window_len = write_pos = 0)
__device__ __forceinline__ void fill_state(const FillPlace& p, int* st) {
    st[0] = p.sl;
    st[1] = p.rem < p.wc ? p.rem : p.wc;
    st[2] = p.rem < p.wc ? p.rem : 0;
    st[3] = p.L;
}

// a packed call with SFA_FLAG_RAGGED_ADMIT (admit != 0): the sequence whose (active) slot has the state row `row` is
// admitted iff the slot is fresh.  The one predicate of the split kernels (get_fill), the commit blocks and the advance.
__device__ __forceinline__ bool admits(int admit, const int* row) { return admit && row[3] == 0; }

// the cache row (and state row) of batch row b: b itself, or slots[b] of a slot call (-1: an inactive row)
template <bool Slots>
__device__ __forceinline__ int cache_row(const MultiArgs& a, int b) {
    if constexpr (!Slots) {
        return b;
    } else {
        const int c = a.slots[b];
        return (unsigned)c < (unsigned)a.npool ? c : -1;
    }
}

// the write slot of cache row c's state, clamped into the ring (dyn); the host state otherwise
__device__ __forceinline__ int state_wp(const MultiArgs& a, int c) {
    if (!a.state) return a.wp;
    const int wp = a.state[(int64_t)c * a.sstride + 2];
    return wp < 0 ? 0 : (wp >= a.wc ? a.wc - 1 : wp);
}

// c: the cache row, wave-uniform (per-sequence state reads row c; a shared state has stride 0)
// Ragged: the chunk length is n (the sequence's own n_i) in place of a.n; admit (the call's flag): a fresh slot
// (seen == 0) reads as an empty cache whatever the other three fields hold, and the first min(n, ns) chunk tokens are
// the sequence's sinks
// Grouped: lg = the shared length of the sequence's group (0: none).  The plan covers the PRIVATE ring slots
// [lg, window_len) alone - ring tile i starts at slot lg + 32 (i - T0), tile_info's roff - while wl and wp stay the
// ring's, for the mask.
// shared (a shared-phase workgroup of the group, c = its first member's row): ring slots [0, lg) as a ring of lg slots
// without sinks and without a chunk, split by a plan of (lg, want_g = the call's shape) alone - every member, whatever
// its own state, folds the same S partials.  One construction of the Fill for both phases.
template <bool Dyn, bool Ragged = false, bool Grouped = false>
__device__ __forceinline__ Fill get_fill(const MultiArgs& a, int c, int n = 0, [[maybe_unused]] int admit = 0,
                                         [[maybe_unused]] int lg = 0, [[maybe_unused]] bool shared = false,
                                         [[maybe_unused]] int want_g = 0) {
    if constexpr (!Dyn) {
        return Fill{a.sink_len, a.wl, a.wp, a.T0, a.T1, a.T, a.tps, a.S, 0};
    } else {
        // dyn mode: the cache state from the device (clamped into the buffers, so that a corrupt state cannot address
        // outside them), replanned.  Wave-uniform: loads of 12 bytes (16 with `seen` in an admitting call), broadcast from
        // the first lane.
        const int* st = a.state + (int64_t)c * a.sstride;
        int sl = __builtin_amdgcn_readfirstlane(st[0]);
        int wl = __builtin_amdgcn_readfirstlane(st[1]);
        int wp = __builtin_amdgcn_readfirstlane(st[2]);
        sl = sl < 0 ? 0 : (sl > a.ns ? a.ns : sl);
        wl = wl < 0 ? 0 : (wl > a.wc ? a.wc : wl);
        wp = wp < 0 ? 0 : (wp >= a.wc ? a.wc - 1 : wp);
        int nsk = 0;
        if constexpr (Ragged) {
            if (__builtin_amdgcn_readfirstlane((int)admits(admit, st))) sl = wl = wp = 0, nsk = n < a.ns ? n : a.ns;
        }
        int pwl = wl;                // the ring slots the plan covers
        [[maybe_unused]] int want = a.want;
        if constexpr (Grouped) {
            pwl = lg < wl ? wl - lg : 0;
            if (shared) sl = 0, wl = lg, wp = 0, nsk = 0, n = 0, pwl = lg, want = want_g;
        }
        const MultiPlan p = multi_plan(sl, pwl, Ragged ? n : a.n, Grouped ? want : a.want);
        auto u = [](int x) { return __builtin_amdgcn_readfirstlane(x); };   // keep the plan in SGPRs
        return Fill{sl, wl, wp, u(p.T0), u(p.T1), u(p.T), u(p.tps), u(p.S), nsk};
    }
}

// the second preparation launch of a grouped call, one workgroup of 1024 threads per group (block g decides group g;
// the two maps are strided over the whole grid).  Unlike ragged_prep_kernel it READS the state rows and the page table:
// the advance of the state is still the trailing launch of the call and the commit blocks run behind the split launch,
// so every reader of a state row or a ring slot still comes before its writer (the state-ordering rule of
// include/sfa.h holds unchanged).
//   gblk: as ragged_prep_kernel's blk with groups in the place of sequences: group g owns the block ids
//         [start_g, start_g + ceil(G n_g / 32)), start_g = floor(G c0_g / 32) + g, below ngrb = ceil(G T / 32) + n_grp;
//   gseq: the last group that starts at or before the sequence, if it covers it;
//   glg:  (Lg, the cache row of the first member).  A MEMBER is an active sequence (slot in the pool) with n_i > 0.
//         Lg = the largest multiple of P such that for every member: it is not admitting; window_len + n_i <= Wc and
//         write_pos == window_len (the ring is unwrapped and stays so within the step: slot = token, every slot visible
//         to every new row); Lg <= window_len; table entries j < Lg / P are mapped and equal the first member's.
//         Fewer than two members: Lg = 0.  A member whose rows leave the group's span (offsets that are not monotonic)
//         makes Lg = 0 too, so that a row that folds group partials is always one a shared-phase workgroup wrote.
//         Groups must not overlap for the same reason (two groups would write the same rows of the group partials
//         under different plans): if the clamped cu_g decreases ANYWHERE, every group of the call gets Lg = 0 and the
//         call computes what the ungrouped one does.
//         The state fields are clamped as get_fill clamps them.  Pass 1: members strided over the threads (limit per
//         member, minimum and first member through LDS; mrow[i] = the member's cache row, -1 for a sequence that is
//         none).  Pass 2: the (member, entry) pairs strided over the threads - 8 members x 1563 entries are 13 rounds,
//         not a serial walk - without a division and without a branch in front of the loads (a round is mrow, then two
//         independent table entries); the first differing entry by an LDS minimum.
__global__ __launch_bounds__(1024) void group_prep_kernel(RaggedArgs rg, GroupArgs gr, PageArgs pg, int2* gblk, int2* glg,
                                                          int* gseq, int* mrow, const int* state, const int* slots,
                                                          int npool, int wc, int G) {
    __shared__ int s_lim, s_first, s_cnt, s_diff, s_bad;
    const int g = blockIdx.x, tid = threadIdx.x;
    for (int x = g * 1024 + tid; x < gr.ngrb + rg.n_seq; x += gridDim.x * 1024) {
        const bool sq = x >= gr.ngrb;
        const int id = sq ? x - gr.ngrb : x;
        int lo = 0, hi = gr.n_grp - 1;       // the last group whose start is at or before the id
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            const GroupSpan s = group_span(rg, gr, mid);
            // an empty group has no rows: it starts where it would lie in the pack, at the first row of sequence i0
            const int c0 = s.n > 0 ? s.c0 : (s.i0 < rg.n_seq ? ragged_seq(rg, s.i0).c0 : rg.T);
            const int64_t start = sq ? s.i0 : (int64_t)G * c0 / 32 + mid;
            if (start <= id) lo = mid;
            else hi = mid - 1;
        }
        const GroupSpan s = group_span(rg, gr, lo);
        if (sq) {
            gseq[id] = (id >= s.i0 && id < s.i1) ? lo : -1;
        } else {
            const int64_t local = id - ((int64_t)G * s.c0 / 32 + lo);
            const bool hit = s.n > 0 && local >= 0 && local * 32 < (int64_t)G * s.n;
            gblk[id] = hit ? make_int2(lo, (int)local) : make_int2(-1, 0);
        }
    }
    if (tid == 0) s_lim = INT_MAX, s_first = INT_MAX, s_cnt = 0, s_diff = INT_MAX, s_bad = 0;
    __syncthreads();
    const GroupSpan sp = group_span(rg, gr, g);
    const int P = 1 << pg.shift;
    for (int x = tid; x < gr.n_grp; x += 1024) {       // offsets that decrease somewhere: groups may overlap
        const int a0 = gr.cu_g[x], a1 = gr.cu_g[x + 1];
        const int b0 = a0 < 0 ? 0 : (a0 > rg.n_seq ? rg.n_seq : a0), b1 = a1 < 0 ? 0 : (a1 > rg.n_seq ? rg.n_seq : a1);
        if (b1 < b0) s_bad = 1;
    }
    for (int i = sp.i0 + tid; i < sp.i1; i += 1024) {
        const int c = slots[i];
        const RaggedSeq s = ragged_seq(rg, i);
        const bool member = (unsigned)c < (unsigned)npool && s.n > 0;
        mrow[i] = member ? c : -1;
        if (!member) continue;                                         // inactive or empty
        const int* st = state + (int64_t)c * 4;
        int wl = st[1], wp = st[2];
        wl = wl < 0 ? 0 : (wl > wc ? wc : wl);
        wp = wp < 0 ? 0 : (wp >= wc ? wc - 1 : wp);
        int lim = wl & ~(P - 1);
        if (admits(rg.admit, st) || wl + s.n > wc || wp != wl) lim = 0;
        if (s.c0 < sp.c0 || s.c0 + s.n > sp.c0 + sp.n) lim = 0;
        atomicMin(&s_lim, lim);
        atomicMin(&s_first, i);
        atomicAdd(&s_cnt, 1);
    }
    __syncthreads();
    const int first = s_first, cnt = s_cnt;
    int lg = cnt >= 2 && !s_bad ? s_lim : 0;
    const int c_first = cnt >= 1 ? slots[first] : 0;
    const int ne = lg >> pg.shift, nm = sp.i1 - sp.i0;
    if (ne > 0) {
        // pair x = (member x / ne, entry x mod ne), x = tid + 1024 round: one division, then steps of 1024 pairs
        const int istep = 1024 / ne, jstep = 1024 - istep * ne;
        int i = sp.i0 + tid / ne, j = tid % ne;
        int diff = INT_MAX;
        for (int64_t x = tid; x < (int64_t)nm * ne; x += 1024) {
            const int c = mrow[i];         // this workgroup wrote it in front of the barrier above
            const int e0 = pg.table[(int64_t)c_first * pg.stride + j];
            const int e = pg.table[(int64_t)(c < 0 ? c_first : c) * pg.stride + j];
            if (c >= 0 && ((unsigned)e0 >= (unsigned)pg.npages || e != e0)) diff = min(diff, j);
            i += istep, j += jstep;
            if (j >= ne) j -= ne, ++i;
        }
        if (diff != INT_MAX) atomicMin(&s_diff, diff);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_diff < ne) lg = s_diff << pg.shift;
        glg[g] = make_int2(lg, c_first);
    }
}

// one 32-key tile: rows [start, start + count) of one segment of the (cache row c / chunk row b, KV head) slice
struct TileInfo {
    const char* k;
    const char* v;
    int64_t ksn, vsn;            // row strides in BYTES
    int seg;                     // 0 sink, 1 ring, 2 chunk
    int start, count;
    int cmin, cmax;              // chronological range of its keys (sink: unused)
};

__device__ __forceinline__ int ring_chron(const MultiArgs& a, const Fill& f, int s) {
    int x = s - f.wp + f.wl;
    if (x >= a.wc) x -= a.wc;
    if (x < 0) x += a.wc;
    return x - f.wl;
}

// Ragged: the chunk is the n rows of k_new / v_new from packed row crow on, in place of the a.n rows of batch row b
// KV8: sink and ring tiles are FP8 rows (1 byte per element); the chunk keeps es
// Paged: a ring tile gets its place inside its page (rows [start mod P, ...) of page 0); tile_page adds the page once
// the tile is known to be live
// roff (a grouped sequence's own workgroups): the first ring slot of the plan, a multiple of P; 0 everywhere else
template <bool Ragged = false, bool KV8 = false, bool Paged = false>
__device__ __forceinline__ TileInfo tile_info(const MultiArgs& a, const Fill& f, int i, int b, int c, int hk, int es,
                                              int n = 0, int crow = 0, [[maybe_unused]] int pshift = 0, int roff = 0) {
    TileInfo ti;
    const View *kv, *vv;
    int len, row = c;            // sink and ring: the cache row; the chunk: the batch row
    if (i < f.T0) {
        ti.seg = 0, ti.start = kTile * i, len = f.sink_len, kv = &a.sk, vv = &a.sv;
    } else if (i < f.T1) {
        ti.seg = 1, ti.start = roff + kTile * (i - f.T0), len = f.wl, kv = &a.wk, vv = &a.wv;
    } else {
        ti.seg = 2, ti.start = kTile * (i - f.T1), len = Ragged ? n : a.n, kv = &a.kn, vv = &a.vn, row = b;
    }
    ti.count = len - ti.start < kTile ? len - ti.start : kTile;
    if constexpr (KV8) es = ti.seg == 2 ? es : 1;
    ti.ksn = kv->sn * es;
    ti.vsn = vv->sn * es;
    int first = ti.start;        // the tile's first row in its buffer
    if constexpr (Paged) {
        if (ti.seg == 1) row = 0, first = ti.start & ((1 << pshift) - 1);
    }
    ti.k = kv->ptr + ((int64_t)row * kv->sb + (int64_t)hk * kv->sh) * es + (int64_t)first * ti.ksn;
    ti.v = vv->ptr + ((int64_t)row * vv->sb + (int64_t)hk * vv->sh) * es + (int64_t)first * ti.vsn;
    if (ti.seg == 2) {
        if constexpr (Ragged) ti.k += (int64_t)crow * ti.ksn, ti.v += (int64_t)crow * ti.vsn;
        ti.cmin = ti.start, ti.cmax = ti.start + ti.count - 1;
    } else if (ti.seg == 1) {
        const int s1 = ti.start + ti.count - 1;
        if (f.wl == a.wc && ti.start < f.wp && f.wp <= s1) ti.cmin = -a.wc, ti.cmax = -1;   // the wrap is inside
        else ti.cmin = ring_chron(a, f, ti.start), ti.cmax = ring_chron(a, f, s1);
    } else {
        ti.cmin = ti.cmax = 0;
    }
    return ti;
}

// a live ring tile of a paged pool: one wave-uniform table lookup (a scalar load, the row and the tile index are in
// SGPRs) moves the tile from page 0 to its page; an unmapped entry stays on page 0 (in bounds, the output unspecified).
// The tile index is the PHYSICAL ring slot start / P: a ring tile has a fixed place in the ring.
// es: bytes per element of the RING (tile_info's local one: 1 in a KV8 instance, whatever the activations have).
__device__ __forceinline__ void tile_page(TileInfo& ti, const MultiArgs& a, const PageArgs& pg, int c, int es) {
    const int e = __builtin_amdgcn_readfirstlane(page_at(pg, c, ti.start));
    const int64_t page = e < 0 ? 0 : e;
    ti.k += page * a.wk.sb * es;
    ti.v += page * a.wv.sb * es;
}

// 0 dead (no row of [tmin, tmax] sees a key), 1 full (every row sees every key), 2 edge
// nsk (Fill): chunk keys c < nsk are sinks, visible behind the window.  A chunk tile that holds one is dead only above
// the diagonal, and full only if its window keys (c >= nsk, if any: nsk is the oldest of them) are in every row's window.
__device__ __forceinline__ int tile_class(const MultiArgs& a, const TileInfo& ti, int tmin, int tmax, int nsk = 0) {
    if (ti.seg == 0) return ti.count == kTile ? 1 : 2;
    if (nsk > 0 && ti.seg == 2 && ti.start < nsk) {   // nsk is the constant 0 outside the ragged instances: no code there
        if (ti.cmin > tmax) return 0;
        return (ti.count == kTile && ti.cmax <= tmin && (ti.cmax < nsk || nsk >= tmax - a.wc + 1)) ? 1 : 2;
    }
    if (ti.cmax < tmin - a.wc + 1 || ti.cmin > tmax) return 0;
    return (ti.count == kTile && ti.cmin >= tmax - a.wc + 1 && ti.cmax <= tmin) ? 1 : 2;
}

__device__ __forceinline__ bool key_visible(const MultiArgs& a, const Fill& f, const TileInfo& ti, int kk, int t) {
    if (kk >= ti.count) return false;
    if (ti.seg == 0) return true;
    const int c = ti.seg == 2 ? ti.start + kk : ring_chron(a, f, ti.start + kk);
    return c <= t && c >= t - a.wc + 1;
}

// a chunk tile of an admitting sequence (f.nsk > 0, ti.seg == 2): chunk keys c < nsk are its sinks, visible behind the
// window.  A separate function so that the loops of every other tile stay the code they were: the callers branch on
// the (wave-uniform) admitting() once per tile, not per element.
__device__ __forceinline__ bool admitting(const Fill& f, const TileInfo& ti) { return f.nsk > 0 && ti.seg == 2; }
__device__ __forceinline__ bool key_visible_admit(const MultiArgs& a, const Fill& f, const TileInfo& ti, int kk, int t) {
    const int c = ti.start + kk;
    return kk < ti.count && c <= t && (c >= t - a.wc + 1 || c < f.nsk);
}

// ---- tree chunks.  Node u sees ring position c iff c >= depth[u] - Wc + 1 and chunk token v iff
// v in anc[u] and depth[u] - depth[v] <= Wc - 1: the chain's mask with the query index replaced by the depth and the
// prefix by the ancestor set.  `vis` is the second set as a bitmask over the chunk (n <= 64).
struct TreeNode {
    int depth;
    uint64_t vis;
};

__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src) {
    const unsigned lo = __shfl((unsigned)x, src), hi = __shfl((unsigned)(x >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// every lane of the wave must call it (cross-lane reads); lane u < n returns node u of batch row b's tree.  One
// coalesced load of parent, then pointer jumping: after round r, j = the 2^r-th ancestor (-1: above the root), d = the
// edges from u up to j (to the root when j = -1), anc = u and its ancestors below j; 6 rounds cover depth 63.  When
// the window clips the chunk (Wc < n), the Wc-th ancestor k is composed from the same jumps (bits of Wc) and
// vis = anc[u] minus anc[k].  An entry outside [-1, u) reads as -1, so a corrupt tree cannot loop or leave the chunk.
// parent: the chunk's n entries (batch row b's tree; the n_i entries of a sequence of a pack), wc: the ring capacity
__device__ __forceinline__ TreeNode tree_node(int n, const int* parent, int wc, int lane) {
    int p = lane < n ? parent[lane] : -1;
    if (p < -1 || p >= lane) p = -1;
    int j = p, d = p >= 0 ? 1 : 0;
    uint64_t anc = 1ull << lane;
    const bool clip = wc < n;            // otherwise depth <= n - 1 <= Wc - 1: every ancestor is in the window
    int kth = lane;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        if (clip && ((wc >> r) & 1)) {
            const int x = __shfl(j, kth < 0 ? lane : kth);
            kth = kth < 0 ? -1 : x;
        }
        const int src = j < 0 ? lane : j;
        const int jj = __shfl(j, src), dd = __shfl(d, src);
        const uint64_t aa = shfl64(anc, src);
        if (j >= 0) d += dd, anc |= aa, j = jj;
    }
    if (clip) {
        const uint64_t ak = shfl64(anc, kth < 0 ? lane : kth);
        if (kth >= 0) anc &= ~ak;
    }
    return TreeNode{d, anc};
}

__device__ __forceinline__ TreeNode tree_node(const MultiArgs& a, int b, int lane) {
    return tree_node(a.n, a.parent + (int64_t)b * a.pstride, a.wc, lane);
}

// packed tree calls (sfa_decode_ring_ragged_tree_slots, the (Tree, Ragged) instances): sequence i of n_i tokens on
// cache row c is a tree sequence iff n_i <= 64 and it is not admitting; its nodes are parent[c0_i .. c0_i + n_i).  Every
// other sequence ignores its entries and takes the ragged mask.  Wave-uniform (n and the state row are).
__device__ __forceinline__ bool ragged_is_tree(const MultiArgs& a, const RaggedArgs& rg, int c, int n) {
    return n <= 64 && !admits(rg.admit, a.state + (int64_t)c * a.sstride);
}

// chunk tiles of a tree call: dead when no row of the block sees a key of the tile (vor = OR of the rows' vis), edge
// otherwise; sink and ring tiles as the chain's, against the block's depth range [dlo, dhi]
template <bool Tree>
__device__ __forceinline__ int tile_class_t(const MultiArgs& a, const TileInfo& ti, int dlo, int dhi, uint64_t vor,
                                            int nsk = 0) {
    if (Tree && ti.seg == 2) {
        const uint64_t m = ti.count >= 64 ? ~0ull : ((1ull << ti.count) - 1);
        return ((vor >> ti.start) & m) ? 2 : 0;
    }
    return tile_class(a, ti, dlo, dhi, nsk);
}

template <bool Tree>
__device__ __forceinline__ bool key_visible_t(const MultiArgs& a, const Fill& f, const TileInfo& ti, int kk, int t,
                                              uint64_t vis) {
    if (Tree && ti.seg == 2) return kk < ti.count && ((vis >> (ti.start + kk)) & 1);
    return key_visible(a, f, ti, kk, t);
}

__device__ __forceinline__ float half_swap_max(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_swap_sum(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// XCD-aware work id (speed only): consecutive block ids land on different XCDs; give each XCD a contiguous range of
// work ids, so that the row blocks of one (batch, KV head, split) - which read the same K/V tiles - share an L2
__device__ __forceinline__ int xcd_work_id(int bid, int nblk) {
    const int q8 = nblk >> 3, r8 = nblk & 7, xcd = bid & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// Ragged (packed calls, with Dyn and Slots): the workgroup's row block comes from the table of ragged_prep_kernel; it
// belongs to ONE sequence, whose length, first packed row and slot become the workgroup's scalars (n, R, prow below),
// and everything else runs as for B = 1.  With Tree the workgroup scalar is_tree (ragged_is_tree) says whether the
// sequence takes the tree prologue, tile classes and chunk mask, or the code a (Ragged, no Tree) instance runs.
// waves_per_eu: the (Tree, Ragged) instance of D = 80 asks for the two waves per SIMD of its tree _slots sibling (the
// allocator then fits it into 226 VGPRs without scratch; left alone it takes 233 + 48 and one wave).  1 = the default of
// every other instance, whose code does not change.
// KV8 (the FP8 pool, with Ragged): sink and ring tiles are loaded as 8-byte pieces - the tile's kTile * CPR chunks of 8
// elements, the lane-to-chunk map unchanged - and converted to T in registers on the way into LDS (kv8_read, the scale
// of head hk: one scalar per workgroup for K and for V); the LDS image and everything behind it are those of the 16-bit
// instance.  Chunk tiles (k_new / v_new) are 16-bit and keep the 16-byte load.
// Paged (the paged pool, with Ragged): a live ring tile takes its page from the table (tile_page) before its loads are
// issued; dead tiles cost no lookup, and everything behind the tile address is the 16-bit instance.
// KV8 and Paged (the paged FP8 pool): both of the above - the lookup in front of the tile address, in bytes of one per
// element, the conversion behind the load.
template <typename T, int D, bool Dyn, bool Tree, bool Slots = false, bool Ragged = false, bool KV8 = false,
          bool Paged = false, typename... RA>
__global__ __launch_bounds__(kWaves * 64) __attribute__((amdgpu_waves_per_eu((Tree && Ragged && D == 80) ? 2 : 1)))
void multi_split_mfma_kernel(MultiArgs a, RA... ra) {
    static_assert(tail_is<Ragged, KV8, Paged, RA...> && !(Ragged && (!Dyn || !Slots)) && !(KV8 && !Ragged) &&
                      !(Paged && !Ragged),
                  "ragged: (MultiArgs, RaggedArgs); FP8 pool: (MultiArgs, RaggedArgs, Kv8Args); paged pool: (MultiArgs, "
                  "RaggedArgs, PageArgs); paged FP8 pool: (MultiArgs, RaggedArgs, Kv8Args, PageArgs)");
    constexpr bool Grouped = has_arg<GroupArgs, RA...>;      // fork groups: the paged forms plus a trailing GroupArgs
    static_assert(!(Grouped && Tree), "no draft trees inside a group");
    [[maybe_unused]] const RaggedArgs& rg = arg_of<RaggedArgs>(ra...);
    [[maybe_unused]] const Kv8Args kv = arg_of<Kv8Args>(ra...);
    [[maybe_unused]] const PageArgs pg = arg_of<PageArgs>(ra...);
    [[maybe_unused]] const GroupArgs& gr = arg_of<GroupArgs>(ra...);
    using M = Mma<T>;
    using frag = typename M::frag;
    constexpr int DK = D / 16;           // k-steps of the K Q^T contraction
    constexpr int DVB = (D + 31) / 32;   // 32-wide output column blocks
    constexpr int CPR = D / 8;           // 16-byte chunks per row
    constexpr int ROWB = D <= 64 ? 128 : 256;
    constexpr int TILE_BYTES = kTile * ROWB;
    constexpr int NLD = kTile * CPR / 64;   // chunks per lane and tile (CPR is even for every served head dim)
    constexpr int DP = D + 1;               // merge rows: padded against bank conflicts
    static_assert(kTile * CPR % 64 == 0, "tile chunks must split evenly over a wave");
    static_assert(2 * kWaves * 32 * 4 + 32 * DP * 4 <= kWaves * 2 * TILE_BYTES, "merge area must fit the tile area");
    __shared__ __attribute__((aligned(16))) char smem[kWaves * 2 * TILE_BYTES];

    // Grouped: block ids [0, nsh) are the shared-phase workgroups (the long ones, so they start first), the rest the
    // members' own; each range gets its own XCD-aware ids (nsh is a multiple of 8: a block's XCD stays bid mod 8)
    int bid = blockIdx.x, nbid = gridDim.x;
    [[maybe_unused]] bool shared = false;
    if constexpr (Grouped) {
        shared = bid < gr.nsh;
        if (shared) nbid = gr.nsh;
        else bid -= gr.nsh, nbid -= gr.nsh;
    }
    const int wid = xcd_work_id(bid, nbid);
    const int nrb_w = Grouped && shared ? gr.ngrb : a.nrb, Sw_w = Grouped && shared ? gr.Sgw : a.Sw;
    int rb = wid % nrb_w;
    int rest = wid / nrb_w;
    const int split = rest % Sw_w;   // decomposition over the LAUNCHED splits
    rest /= Sw_w;
    const int hk = rest % a.Hkv;
    const int b = rest / a.Hkv;
    if (Grouped && b > 0) return;      // the padding of nsh (a pack has B = 1)
    int c = b;                         // the cache row: per workgroup, in an SGPR
    // ragged: the sequence's length, rows and first packed row (in place of a.n, a.R and batch row b)
    [[maybe_unused]] int rn = 0, rR = 0, prow = 0;
    // grouped: the shared length of the workgroup's group (0: the sequence is in none, or its group shares nothing)
    [[maybe_unused]] int lg = 0;
    const auto nrow = [&]() { if constexpr (Ragged) return rR; else return a.R; };
    if constexpr (Ragged) {
        if (Grouped && shared) {
            // a shared-phase workgroup: (group, 32-row block of the group's rows, KV head, group split).  Its rows are
            // the group's packed rows as ONE virtual sequence, its keys ring slots [0, lg) of the first member's pages
            const int2 e = gr.gblk[rb];
            const int g = __builtin_amdgcn_readfirstlane(e.x);
            if (g < 0) return;         // surplus of the group row-block bound
            rb = __builtin_amdgcn_readfirstlane(e.y);
            const int2 gl = gr.glg[g];
            lg = __builtin_amdgcn_readfirstlane(gl.x);
            if (lg <= 0) return;       // nothing shared: the members read everything themselves
            c = __builtin_amdgcn_readfirstlane(gl.y);
            const GroupSpan sp = group_span(rg, gr, g);
            prow = __builtin_amdgcn_readfirstlane(sp.c0);
            rn = __builtin_amdgcn_readfirstlane(sp.n);
            rR = a.G * rn;
        } else {
            const int2 e = rg.blk[rb];
            const int seq = __builtin_amdgcn_readfirstlane(e.x);
            if (seq < 0) return;           // surplus of the row-block bound (whole workgroup)
            rb = __builtin_amdgcn_readfirstlane(e.y);
            c = __builtin_amdgcn_readfirstlane(cache_row<true>(a, seq));
            if (c < 0) return;             // inactive sequence: the reduce writes its zeros
            const RaggedSeq s = ragged_seq(rg, seq);
            prow = __builtin_amdgcn_readfirstlane(s.c0);
            rn = __builtin_amdgcn_readfirstlane(s.n);
            rR = a.G * rn;
            if constexpr (Grouped) {
                const int g = __builtin_amdgcn_readfirstlane(gr.gseq[seq]);
                if (g >= 0) lg = __builtin_amdgcn_readfirstlane(gr.glg[g].x);
            }
        }
    } else if constexpr (Slots) {
        c = __builtin_amdgcn_readfirstlane(cache_row<true>(a, b));
        if (c < 0) return;             // inactive row (whole workgroup): the reduce writes its zeros
    }
    const Fill f = get_fill<Dyn, Ragged, Grouped>(a, c, rn, rg.admit, lg, shared, gr.want_g);
    if (Dyn && split >= f.S) return;   // surplus of the full-cache grid at this fill level (whole workgroup)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int rho = 32 * rb + r;
    const bool row_live = rho < nrow();
    const int tq = row_live ? rho / a.G : 0;            // the lane's query index (dead rows: any, never stored)
    int tmin = (32 * rb) / a.G;
    int tmax = ((32 * rb + 31 < nrow() - 1) ? 32 * rb + 31 : nrow() - 1) / a.G;
    // tree: the lane's row is node tq at depth td; [tmin, tmax] becomes the block's depth range over its live rows
    int td = tq;
    uint64_t tvis = 0, vor = 0;
    // a pack: per sequence (the whole workgroup takes one side)
    [[maybe_unused]] bool is_tree = Tree;
    if constexpr (Tree && Ragged) is_tree = __builtin_amdgcn_readfirstlane((int)ragged_is_tree(a, rg, c, rn)) != 0;
    if (Tree && is_tree) {
        TreeNode me;
        if constexpr (Ragged) me = tree_node(rn, a.parent + prow, a.wc, lane);
        else me = tree_node(a, b, lane);
        // every lane runs the cross-lane reads (a source lane masked off by a branch would read as 0), then selects
        td = __shfl(me.depth, tq);
        const uint64_t v = shfl64(me.vis, tq);
        tvis = row_live ? v : 0;
        int lo = row_live ? td : INT_MAX, hi = row_live ? td : -1;
        vor = tvis;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            lo = min(lo, __shfl_xor(lo, s));
            hi = max(hi, __shfl_xor(hi, s));
            vor |= shfl64(vor, lane ^ s);
        }
        tmin = __builtin_amdgcn_readfirstlane(lo);   // wave-uniform: keep the tile classification scalar
        tmax = __builtin_amdgcn_readfirstlane(hi);
        vor = ((uint64_t)__builtin_amdgcn_readfirstlane((unsigned)(vor >> 32)) << 32) |
              (unsigned)__builtin_amdgcn_readfirstlane((unsigned)vor);
    }

    // ---- Q fragments: B operand of X^T = K Q^T; lane (r, h) holds Q[row r][16 ks + 8 h .. +8)
    frag qf[DK];
    {
        const int head = hk * a.G + (row_live ? rho % a.G : 0);
        const char* qp = a.q.ptr + ((int64_t)b * a.q.sb + (int64_t)head * a.q.sh + (int64_t)(Ragged ? prow + tq : tq) * a.q.sn) * 2;
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) {
            u32x4 raw = *reinterpret_cast<const u32x4*>(qp + (2 * ks + h) * 16);
            if (!row_live) raw = u32x4{0u, 0u, 0u, 0u};
            qf[ks] = __builtin_bit_cast(frag, raw);
        }
    }

    char* kl = smem + wave * 2 * TILE_BYTES;
    char* vl = kl + TILE_BYTES;
    u32x4 kst[NLD], vst[NLD];
    // FP8 pool: the K and V scales of head hk (wave-uniform) and whether the staged tile holds codes (kst / vst [0..1])
    [[maybe_unused]] float ksc = 1.f, vsc = 1.f;
    [[maybe_unused]] bool st8 = false;
    if constexpr (KV8) ksc = kv8_scale(kv, 0, a.Hkv, hk), vsc = kv8_scale(kv, 1, a.Hkv, hk);
    auto issue_loads = [&](const TileInfo& ti) {
        if constexpr (KV8) {
            st8 = ti.seg != 2;
            if (st8) {
#pragma unroll
                for (int j = 0; j < NLD; ++j) {
                    const int c = lane + 64 * j;
                    const int key = c / CPR, ch = c % CPR;
                    const int row = key < ti.count ? key : ti.count - 1;
                    const uint2 k8 = *reinterpret_cast<const uint2*>(ti.k + row * ti.ksn + ch * 8);
                    const uint2 v8 = *reinterpret_cast<const uint2*>(ti.v + row * ti.vsn + ch * 8);
                    kst[j][0] = k8.x, kst[j][1] = k8.y, vst[j][0] = v8.x, vst[j][1] = v8.y;
                }
                return;
            }
        }
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int c = lane + 64 * j;
            const int key = c / CPR, ch = c % CPR;
            const int row = key < ti.count ? key : ti.count - 1;   // rows past the segment: a valid row, masked later
            kst[j] = *reinterpret_cast<const u32x4*>(ti.k + row * ti.ksn + ch * 16);
            vst[j] = *reinterpret_cast<const u32x4*>(ti.v + row * ti.vsn + ch * 16);
        }
    };
    auto write_lds = [&]() {
        if constexpr (KV8) {
            if (st8) {                 // the conversion: between the global load and the LDS store
#pragma unroll
                for (int j = 0; j < NLD; ++j) {
                    kst[j] = kv8_read<T>(kst[j][0], kst[j][1], ksc);
                    vst[j] = kv8_read<T>(vst[j][0], vst[j][1], vsc);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int c = lane + 64 * j;
            const int key = c / CPR, ch = c % CPR;
            const int ksw = ROWB == 256 ? (key & 15) : ((key >> 1) & 7);
            const int vsw = ROWB == 256 ? ((key & 3) << 2) : (((key >> 1) & 1) << 2);
            *reinterpret_cast<u32x4*>(kl + key * ROWB + ((ch ^ ksw) << 4)) = kst[j];
            *reinterpret_cast<u32x4*>(vl + key * ROWB + ((ch ^ vsw) << 4)) = vst[j];
        }
    };

    // per-lane LDS read addressing (kh = 0 of the forward kernel's 64-key tile)
    const int ksw_l = ROWB == 256 ? (r & 15) : ((r >> 1) & 7);
    const int k_rowoff = r * ROWB;
    const int q4 = (lane & 15) >> 2, p4 = lane & 3, g1 = (lane >> 4) & 1;
    const int vsw_l = ROWB == 256 ? (q4 << 2) : (((q4 >> 1) & 1) << 2);
    const int v_rowoff = (4 * h + q4) * ROWB + (p4 & 1) * 8;
    const int v_chunk_lo = 2 * g1 + (p4 >> 1);

    float m = -INFINITY, l = 0.f;   // log2 domain; l: this half-wave's partial sum
    f32x16 o[DVB];
#pragma unroll
    for (int db = 0; db < DVB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[db][i] = 0.f;
    const float c2 = a.scale_log2;
    const int es = 2;

    const int tbeg = split * f.tps;
    const int tend = tbeg + f.tps < f.T ? tbeg + f.tps : f.T;
    auto next_live = [&](int i, TileInfo& ti, int& cls) {
        for (; i < tend; i += kWaves) {
            // Grouped: a member's private ring slots start at lg; the shared phase walks ring tiles of [0, lg) only
            if constexpr (Grouped) ti = tile_info<Ragged, KV8, Paged>(a, f, i, b, c, hk, es, rn, prow, pg.shift, shared ? 0 : lg);
            else ti = tile_info<Ragged, KV8, Paged>(a, f, i, b, c, hk, es, rn, prow, pg.shift);
            if (Tree && Ragged && !is_tree) cls = tile_class(a, ti, tmin, tmax, f.nsk);
            else cls = tile_class_t<Tree>(a, ti, tmin, tmax, vor, f.nsk);
            if constexpr (Grouped) {
                if (shared) cls = 1;   // every shared tile is of class full: no sink tile, no chunk tile, no mask
            }
            if (cls != 0) break;
        }
        if constexpr (Paged) {
            if (i < tend && ti.seg == 1) tile_page(ti, a, pg, c, KV8 ? 1 : es);
        }
        return i;
    };
    TileInfo cur, nxt;
    int ccls = 0, ncls = 0;
    int ic = next_live(tbeg + wave, cur, ccls);
    if (ic < tend) {
        issue_loads(cur);
        write_lds();
    }
    while (ic < tend) {
        const int in = next_live(ic + kWaves, nxt, ncls);
        if (in < tend) issue_loads(nxt);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this tile's LDS writes landed (the wave reads other lanes' rows)

        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
        {
            frag kf[DK];
#pragma unroll
            for (int ks = 0; ks < DK; ++ks) kf[ks] = *reinterpret_cast<const frag*>(kl + k_rowoff + (((2 * ks + h) ^ ksw_l) << 4));
#pragma unroll
            for (int ks = 0; ks < DK; ++ks) s = M::run(kf[ks], qf[ks], s);
        }
        if (Ragged && ccls == 2 && admitting(f, cur)) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kk = (i & 3) + 8 * (i >> 2) + 4 * h;
                s[i] = key_visible_admit(a, f, cur, kk, td) ? s[i] : -INFINITY;
            }
        } else if (Tree && Ragged && ccls == 2 && !(is_tree && cur.seg == 2)) {
            // a tile outside a tree's chunk: the ragged instance's loop (td = the depth for a tree sequence)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kk = (i & 3) + 8 * (i >> 2) + 4 * h;
                s[i] = key_visible(a, f, cur, kk, td) ? s[i] : -INFINITY;
            }
        } else if (ccls == 2) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kk = (i & 3) + 8 * (i >> 2) + 4 * h;
                s[i] = key_visible_t<Tree>(a, f, cur, kk, td, tvis) ? s[i] : -INFINITY;
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, s[i]);
        mx = half_swap_max(mx);
        const float m_new = fmaxf(m, mx * c2);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m - m_safe);
        float rs = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            s[i] = __builtin_amdgcn_exp2f(fmaf(s[i], c2, -m_safe));
            rs += s[i];
        }
        l = fmaf(l, alpha, rs);
        m = m_new;
#pragma unroll
        for (int db = 0; db < DVB; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
        // O^T += V^T X^T: the exponentiated accumulator is the B operand (k index = key, permuted as in the forward)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            frag pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (typename M::elem)s[8 * st + j];
            const char* vrow = vl + 16 * st * ROWB + v_rowoff;
#pragma unroll
            for (int db = 0; db < DVB; ++db) {
                const int ch = (4 * db + v_chunk_lo) ^ vsw_l;
                const char* p1 = vrow + (ch << 4);
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p1));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p1 + 8 * ROWB));
                s16x8 vv;
                vv[0] = lo[0]; vv[1] = lo[1]; vv[2] = lo[2]; vv[3] = lo[3];
                vv[4] = hi[0]; vv[5] = hi[1]; vv[6] = hi[2]; vv[7] = hi[3];
                o[db] = M::run(__builtin_bit_cast(frag, vv), pf, o[db]);
            }
        }
        if (in < tend) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every LDS read of this tile returned before the overwrite
            write_lds();
        }
        ic = in;
        cur = nxt;
        ccls = ncls;
    }

    // ---- merge the 4 waves' (m, l, O) in wave order through LDS (the tile area is free after the barrier)
    const float lw = half_swap_sum(l);
    __syncthreads();
    float* sm = reinterpret_cast<float*>(smem);      // [wave][32]
    float* sl = sm + kWaves * 32;                    // [wave][32]
    float* so = sl + kWaves * 32;                    // [32][DP]
    if (h == 0) {
        sm[wave * 32 + r] = m;
        sl[wave * 32 + r] = lw;
    }
    __syncthreads();
    float mstar = -INFINITY;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) mstar = fmaxf(mstar, sm[w * 32 + r]);
    const float wgt = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mstar);
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int db = 0; db < DVB; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int col = 32 * db + 8 * (i >> 2) + 4 * h + (i & 3);
                    if (col < D) {
                        float* p = so + r * DP + col;
                        *p = (w == 0 ? 0.f : *p) + o[db][i] * wgt;
                    }
                }
        }
        __syncthreads();
    }
    // partial row of the block's first row
    const int64_t row0 = Ragged ? ((int64_t)hk * rg.T + prow) * a.G + 32 * rb : ((int64_t)b * a.Hkv + hk) * a.R + 32 * rb;
    const int nrows = nrow() - 32 * rb < 32 ? nrow() - 32 * rb : 32;
    // one partial per row and split: [rows][Sw] of m and l, [rows][Sw][D] of O.  The same statements as the ungrouped
    // stores below, which stay as they are for the resource records of the existing instances: change both together
    [[maybe_unused]] auto store_partials = [&](float* Mp, float* Lp, float* Op, int Sw) {
        if (tid < nrows) {
            float ms = -INFINITY;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) ms = fmaxf(ms, sm[w * 32 + tid]);
            float lt = 0.f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const float mw = sm[w * 32 + tid];
                lt += mw == -INFINITY ? 0.f : sl[w * 32 + tid] * __builtin_amdgcn_exp2f(mw - ms);
            }
            Mp[(row0 + tid) * Sw + split] = ms;
            Lp[(row0 + tid) * Sw + split] = lt;
        }
        for (int e = tid; e < nrows * D; e += kWaves * 64) {
            const int rr = e / D, d = e - rr * D;
            Op[((row0 + rr) * Sw + split) * D + d] = so[rr * DP + d];
        }
    };
    if constexpr (Grouped) {           // the same rows; a shared-phase workgroup writes the group's area with its stride
        if (shared) store_partials(gr.Mg, gr.Lg, gr.Og, gr.Sgw);
        else store_partials(a.Mp, a.Lp, a.Op, a.Sw);
        return;
    }
    if (tid < nrows) {
        float ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) ms = fmaxf(ms, sm[w * 32 + tid]);
        float lt = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const float mw = sm[w * 32 + tid];
            lt += mw == -INFINITY ? 0.f : sl[w * 32 + tid] * __builtin_amdgcn_exp2f(mw - ms);
        }
        a.Mp[(row0 + tid) * a.Sw + split] = ms;
        a.Lp[(row0 + tid) * a.Sw + split] = lt;
    }
    for (int e = tid; e < nrows * D; e += kWaves * 64) {
        const int rr = e / D, d = e - rr * D;
        a.Op[((row0 + rr) * a.Sw + split) * D + d] = so[rr * DP + d];
    }
}

// a packed (ragged) partial row: rowid = (hk * T + packed row) * G + g.  Finds the row's sequence in the table: the
// callers go on as for B = 1 with rho = the row within the sequence, n = its length and c0 = its first packed row.
// False: the row has no work (padding, an empty or inactive sequence); rho = the query head within the group and tp =
// the packed row then say where its zeros go.
struct RaggedRow {
    int rho, hk, c, tp, n, c0;
};

__device__ __forceinline__ bool ragged_row(const MultiArgs& a, const RaggedArgs& rg, int64_t rowid, RaggedRow& r) {
    const int64_t per = (int64_t)rg.T * a.G;
    r.hk = (int)(rowid / per);
    const int pr = (int)(rowid % per);
    r.tp = pr / a.G;
    r.rho = pr % a.G;
    r.c = -1, r.n = 0, r.c0 = 0;
    const int seq = __builtin_amdgcn_readfirstlane(rg.rowseq[r.tp]);
    if (seq < 0) return false;
    r.c = __builtin_amdgcn_readfirstlane(cache_row<true>(a, seq));
    if (r.c < 0) return false;
    const RaggedSeq s = ragged_seq(rg, seq);
    r.c0 = __builtin_amdgcn_readfirstlane(s.c0);
    r.n = __builtin_amdgcn_readfirstlane(s.n);
    r.rho += (r.tp - r.c0) * a.G;
    return true;
}

// f32-accumulate path: one wave per (partial row, split); lane owns columns lane + 64 j.  Keys one at a time.
template <typename T, bool Dyn, bool Tree, bool Slots = false, bool Ragged = false, typename... RA>
__global__ __launch_bounds__(256) void multi_split_f32_kernel(MultiArgs a, RA... ra) {
    static_assert(tail_is<Ragged, false, false, RA...> && !(Ragged && (!Dyn || !Slots)), "ragged: (MultiArgs, RaggedArgs)");
    [[maybe_unused]] const RaggedArgs& rg = arg_of<RaggedArgs>(ra...);
    constexpr int MAXJ = 8;   // D <= 512 (1 KiB rows of 16-bit types; fp32 stops at 256)
    const int lane = threadIdx.x & 63;
    const int64_t rowid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int split = blockIdx.y;
    const int64_t nrow = Ragged ? (int64_t)a.Hkv * rg.T * a.G : (int64_t)a.B * a.Hkv * a.R;
    if (rowid >= nrow) return;
    int rho = (int)(rowid % a.R);
    int hk = (int)((rowid / a.R) % a.Hkv);
    const int b = Ragged ? 0 : (int)(rowid / ((int64_t)a.R * a.Hkv));
    // per wave: with R < 4 one workgroup holds rows of different sequences, and each has its own fill (and slot)
    int c = b;
    [[maybe_unused]] int rn = 0, prow = 0;    // ragged: the sequence's length and first packed row
    if constexpr (Ragged) {
        RaggedRow r;
        if (!ragged_row(a, rg, rowid, r)) return;
        rho = r.rho, hk = r.hk, c = r.c, rn = r.n, prow = r.c0;
    } else if constexpr (Slots) {
        c = __builtin_amdgcn_readfirstlane(cache_row<true>(a, b));
        if (c < 0) return;
    }
    const Fill f = get_fill<Dyn, Ragged>(a, c, rn, rg.admit);
    if (Dyn && split >= f.S) return;
    const int t = rho / a.G, head = hk * a.G + rho % a.G;
    const int D = a.D;
    const int es = (int)sizeof(T);
    const T* qp = reinterpret_cast<const T*>(a.q.ptr + ((int64_t)b * a.q.sb + (int64_t)head * a.q.sh + (int64_t)(Ragged ? prow + t : t) * a.q.sn) * es);
    float qf[MAXJ], acc[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int d = lane + 64 * j;
        qf[j] = d < D ? to_f32(qp[d]) * a.scale_log2 : 0.f;
        acc[j] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    int td = t;   // tree: the row's node t at depth td, chunk keys vis (wave-uniform)
    uint64_t vis = 0;
    // a pack: per sequence, so per wave (ragged_is_tree)
    [[maybe_unused]] bool is_tree = Tree;
    if constexpr (Tree && Ragged) is_tree = __builtin_amdgcn_readfirstlane((int)ragged_is_tree(a, rg, c, rn)) != 0;
    if (Tree && is_tree) {
        TreeNode me;
        if constexpr (Ragged) me = tree_node(rn, a.parent + prow, a.wc, lane);
        else me = tree_node(a, b, lane);
        td = __builtin_amdgcn_readfirstlane(__shfl(me.depth, t));
        const uint64_t v = shfl64(me.vis, t);
        vis = ((uint64_t)__builtin_amdgcn_readfirstlane((unsigned)(v >> 32)) << 32) |
              (unsigned)__builtin_amdgcn_readfirstlane((unsigned)v);
    }
    const int tbeg = split * f.tps;
    const int tend = tbeg + f.tps < f.T ? tbeg + f.tps : f.T;
    for (int i = tbeg; i < tend; ++i) {
        const TileInfo ti = tile_info<Ragged>(a, f, i, b, c, hk, es, rn, prow);
        if ((Tree && Ragged && !is_tree ? tile_class(a, ti, td, td, f.nsk) : tile_class_t<Tree>(a, ti, td, td, vis, f.nsk)) == 0) continue;
        const bool adm = Ragged && admitting(f, ti);
        const bool plain = Tree && Ragged && !is_tree;      // a chain or admitting sequence of a packed tree call
        for (int kk = 0; kk < ti.count; ++kk) {
            if (!(adm     ? key_visible_admit(a, f, ti, kk, td)
                  : plain ? key_visible(a, f, ti, kk, td)
                          : key_visible_t<Tree>(a, f, ti, kk, td, vis)))
                continue;
            const T* kp = reinterpret_cast<const T*>(ti.k + kk * ti.ksn);
            const T* vp = reinterpret_cast<const T*>(ti.v + kk * ti.vsn);
            float x = 0.f;
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) {
                const int d = lane + 64 * j;
                if (d < D) x = fmaf(qf[j], to_f32(kp[d]), x);
            }
            x = wave_sum(x);   // a butterfly: every lane ends with the same bits
            const float m_new = fmaxf(m, x);
            const float alpha = exp2f(m - m_new);   // m = -inf at the first key: 0
            const float p = exp2f(x - m_new);
            l = l * alpha + p;
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) {
                const int d = lane + 64 * j;
                if (d < D) acc[j] = fmaf(p, to_f32(vp[d]), acc[j] * alpha);
            }
            m = m_new;
        }
    }
    if (lane == 0) {
        a.Mp[rowid * a.Sw + split] = m;
        a.Lp[rowid * a.Sw + split] = l;
    }
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int d = lane + 64 * j;
        if (d < D) a.Op[(rowid * a.Sw + split) * D + d] = acc[j];
    }
}

__device__ __forceinline__ int clamp_count(const int* count, int n) {
    const int c = *count;
    return c < 0 ? 0 : (c > n ? n : c);
}

// one 16-byte piece of the commit: item = ((b * Hkv + hk) * nslot + j) * cpr + ch over the nslot = min(n, Wc) chunk
// tokens a commit can store.  Row b stores acc = clamp(count, 0, n) tokens (all n without a count): piece j is chunk
// token first + j with first = max(0, acc - Wc), stored only if < acc -> ring slot (write_pos + t) mod Wc, write_pos
// of row b's state.  count: one value shared by the batch, or [B] with per-sequence state.
// Path: the j-th stored token is chunk row path[b * pathstride + j] (clamped into [0, n)) instead of row j.
// Slots: ring and state are those of cache row slots[b] (an inactive row stores nothing); chunk, count and path stay on b.
template <bool Path = false, bool Slots = false>
__device__ __forceinline__ void commit_piece(const MultiArgs& a, int64_t item, int es, const int* count) {
    const int cpr = a.D * es / 16;
    const int nslot = a.n < a.wc ? a.n : a.wc;
    if (item >= (int64_t)a.B * a.Hkv * nslot * cpr) return;
    const int ch = (int)(item % cpr);
    int64_t rest = item / cpr;
    const int j = (int)(rest % nslot);
    rest /= nslot;
    const int hk = (int)(rest % a.Hkv);
    const int b = (int)(rest / a.Hkv);
    const int c = cache_row<Slots>(a, b);
    if (Slots && c < 0) return;
    const int last = count ? clamp_count(count + (a.sstride ? b : 0), a.n) : a.n;
    const int t = (last > a.wc ? last - a.wc : 0) + j;
    if (t >= last) return;
    const int slot = (int)(((int64_t)state_wp(a, c) + t) % a.wc);
    int src = t;
    if constexpr (Path) {
        src = a.path[(int64_t)b * a.pathstride + t];
        src = src < 0 ? 0 : (src >= a.n ? a.n - 1 : src);
    }
    const int64_t so = (int64_t)ch * 16;
    const char* ks = a.kn.ptr + ((int64_t)b * a.kn.sb + (int64_t)hk * a.kn.sh + (int64_t)src * a.kn.sn) * es + so;
    const char* vs = a.vn.ptr + ((int64_t)b * a.vn.sb + (int64_t)hk * a.vn.sh + (int64_t)src * a.vn.sn) * es + so;
    char* kd = a.wk.ptr + ((int64_t)c * a.wk.sb + (int64_t)hk * a.wk.sh + (int64_t)slot * a.wk.sn) * es + so;
    char* vd = a.wv.ptr + ((int64_t)c * a.wv.sb + (int64_t)hk * a.wv.sh + (int64_t)slot * a.wv.sn) * es + so;
    *reinterpret_cast<u32x4*>(kd) = *reinterpret_cast<const u32x4*>(ks);
    *reinterpret_cast<u32x4*>(vd) = *reinterpret_cast<const u32x4*>(vs);
}

// the commit piece of a packed call: item = (hk * T + packed row) * cpr + ch.  The row is token t of its sequence i
// (n_i tokens, slot c): stored iff t >= n_i - Wc, into ring slot (write_pos_c + t) mod Wc - what commit_piece<false, true>
// stores for a batch row of n_i tokens.  Rows of no sequence and of inactive sequences store nothing.
// An admitting sequence (admits()) takes the prefill placement instead: token t goes to row fill_dst of its slot.
// A sequence whose commit_seq entry is 0 stores nothing.
// Q (store_piece): void, or the chunk's 16-bit type when the pool is FP8 - es stays the chunk's element size, a piece 8
// elements.
// Paged: a ring slot is stored into row slot mod P of its page (page_at); a slot on an unmapped page is dropped.
template <typename Q, bool Paged>
__device__ __forceinline__ void commit_piece_ragged(const MultiArgs& a, const RaggedArgs& rg, int64_t item, int es,
                                                    const Kv8Args& kv, [[maybe_unused]] const PageArgs& pg) {
    const int cpr = a.D * es / 16;
    if (item >= (int64_t)a.Hkv * rg.T * cpr) return;
    const int ch = (int)(item % cpr);
    const int64_t rest = item / cpr;
    const int tp = (int)(rest % rg.T);
    const int hk = (int)(rest / rg.T);
    const int seq = rg.rowseq[tp];
    if (seq < 0) return;
    if (rg.commit_seq && !rg.commit_seq[seq]) return;
    const int c = cache_row<true>(a, seq);
    if (c < 0) return;
    const RaggedSeq s = ragged_seq(rg, seq);
    const int t = tp - s.c0;
    const View *dk = &a.wk, *dv = &a.wv;
    int slot;
    if (admits(rg.admit, a.state + (int64_t)c * a.sstride)) {
        const int j = fill_dst(fill_place(s.n, a.ns, a.wc), t);
        if (j < 0) return;
        if (j < a.ns) slot = j, dk = &a.sk, dv = &a.sv;
        else slot = j - a.ns;
    } else {
        if (t < s.n - a.wc) return;
        slot = (int)(((int64_t)state_wp(a, c) + t) % a.wc);
    }
    int drow = c;                // the destination's row of its buffer: the cache row, or the page of a ring slot
    if constexpr (Paged) {
        if (dk == &a.wk) {
            if ((drow = page_at(pg, c, slot)) < 0) return;
            slot = page_row(pg, slot);
        }
    }
    const int64_t so = (int64_t)ch * 16, dso = piece_off<Q>(ch);
    const int ed = piece_es<Q>(es);
    const char* ks = a.kn.ptr + ((int64_t)hk * a.kn.sh + (int64_t)tp * a.kn.sn) * es + so;
    const char* vs = a.vn.ptr + ((int64_t)hk * a.vn.sh + (int64_t)tp * a.vn.sn) * es + so;
    char* kd = dk->ptr + ((int64_t)drow * dk->sb + (int64_t)hk * dk->sh + (int64_t)slot * dk->sn) * ed + dso;
    char* vd = dv->ptr + ((int64_t)drow * dv->sb + (int64_t)hk * dv->sh + (int64_t)slot * dv->sn) * ed + dso;
    store_piece<Q>(kd, vd, ks, vs, kv, a.Hkv, hk);
}

// blocks [0, nred): one wave per partial row folds the S partials and s_aux, writes o.  Blocks [nred, ...) with commit:
// store chunk tokens t >= n - Wc into ring slot (write_pos + t) mod Wc, one 16-byte piece of K and of V per thread.
// Dyn: S and write_pos come from the device state (which this launch only reads; ring_advance_kernel moves it on).
// With per-sequence state both are row b's: S per wave (a workgroup can hold rows of different sequences), write_pos
// per commit piece.
// Slots: S, write_pos and the ring are those of cache row slots[b]; an inactive row gets zeros in o (no partial of it
// was written) and stores nothing.
// Ragged: rows are the packed rows (ragged_row); a row without work gets zeros, the commit is commit_piece_ragged.
// KV8 (the FP8 pool, with Ragged): the commit blocks quantise as they store; the fold is the 16-bit instance's.
// Paged (the paged pool, with Ragged): the commit blocks store through the page table; the fold reads no cache.
// KV8 and Paged: the commit blocks quantise as they store through the table.
template <typename T, bool Dyn, bool Slots = false, bool Ragged = false, bool KV8 = false, bool Paged = false, typename... RA>
__global__ __launch_bounds__(256) void multi_reduce_kernel(MultiArgs a, int nred, RA... ra) {
    static_assert(tail_is<Ragged, KV8, Paged, RA...> && !(Ragged && (!Dyn || !Slots)) && !(KV8 && !Ragged) &&
                      !(Paged && !Ragged),
                  "ragged: (MultiArgs, nred, RaggedArgs); FP8 pool: (..., Kv8Args); paged pool: (..., PageArgs); paged FP8 "
                  "pool: (..., Kv8Args, PageArgs)");
    constexpr bool Grouped = has_arg<GroupArgs, RA...>;      // fork groups: the paged forms plus a trailing GroupArgs
    [[maybe_unused]] const RaggedArgs& rg = arg_of<RaggedArgs>(ra...);
    const int es = (int)sizeof(T);
    if ((int)blockIdx.x >= nred) {
        const int64_t item = (int64_t)(blockIdx.x - nred) * 256 + threadIdx.x;
        if constexpr (Ragged)
            commit_piece_ragged<std::conditional_t<KV8, T, void>, Paged>(a, rg, item, es, arg_of<Kv8Args>(ra...), arg_of<PageArgs>(ra...));
        else commit_piece<false, Slots>(a, item, es, nullptr);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int64_t rowid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rowid >= (Ragged ? (int64_t)a.Hkv * rg.T * a.G : (int64_t)a.B * a.Hkv * a.R)) return;
    int rho = (int)(rowid % a.R);
    int hk = (int)((rowid / a.R) % a.Hkv);
    const int b = Ragged ? 0 : (int)(rowid / ((int64_t)a.R * a.Hkv));
    int c = b;
    [[maybe_unused]] int rn = 0, prow = 0;    // ragged: the sequence's length and first packed row
    if constexpr (Ragged) {
        RaggedRow r;
        if (!ragged_row(a, rg, rowid, r)) {
            T* orow = reinterpret_cast<T*>(a.o.ptr + ((int64_t)(r.hk * a.G + r.rho) * a.o.sh + (int64_t)r.tp * a.o.sn) * es);
            for (int d = lane; d < a.D; d += 64) orow[d] = from_f32<T>(0.f);
            return;
        }
        rho = r.rho, hk = r.hk, c = r.c, rn = r.n, prow = r.c0;
    }
    const int t = rho / a.G, head = hk * a.G + rho % a.G;
    if constexpr (Slots && !Ragged) {
        c = __builtin_amdgcn_readfirstlane(cache_row<true>(a, b));
        if (c < 0) {
            T* orow = reinterpret_cast<T*>(a.o.ptr + ((int64_t)b * a.o.sb + (int64_t)head * a.o.sh + (int64_t)t * a.o.sn) * es);
            for (int d = lane; d < a.D; d += 64) orow[d] = from_f32<T>(0.f);
            return;
        }
    }
    // Grouped: a row of a sequence whose group shares lg > 0 ring slots folds its own S partials (the plan of its private
    // part), then its group's Sg (the plan of (lg, the call's shape)), then s_aux - a fixed order, the same butterflies
    [[maybe_unused]] int lg = 0, Sg = 0;
    [[maybe_unused]] const GroupArgs& gr = arg_of<GroupArgs>(ra...);
    if constexpr (Grouped) {
        const int g = __builtin_amdgcn_readfirstlane(gr.gseq[rg.rowseq[prow + t]]);
        if (g >= 0) lg = __builtin_amdgcn_readfirstlane(gr.glg[g].x);
        if (lg > 0) Sg = multi_plan(0, lg, 0, gr.want_g).S;
    }
    const Fill f = get_fill<Dyn, Ragged, Grouped>(a, c, rn, rg.admit, lg);
    const int S = f.S, D = a.D;
    const float* Mr = a.Mp + rowid * a.Sw;
    const float* Lr = a.Lp + rowid * a.Sw;
    const float* Or = a.Op + rowid * a.Sw * D;
    [[maybe_unused]] const float *Mgr = nullptr, *Lgr = nullptr, *Ogr = nullptr;
    if constexpr (Grouped) Mgr = gr.Mg + rowid * gr.Sgw, Lgr = gr.Lg + rowid * gr.Sgw, Ogr = gr.Og + rowid * gr.Sgw * D;
    const float sa = a.s_aux ? a.s_aux[head] * kLog2e : -INFINITY;
    // split statistics spread over the lanes (latency-bound: one round of loads, not S dependent ones), folded by the
    // fixed butterflies of wave_max / wave_sum
    float mloc = -INFINITY;
    for (int s = lane; s < S; s += 64) mloc = fmaxf(mloc, Mr[s]);
    if constexpr (Grouped)
        for (int s = lane; s < Sg; s += 64) mloc = fmaxf(mloc, Mgr[s]);
    const float mstar = fmaxf(wave_max(mloc), sa);   // finite: every row sees at least its own token
    float lloc = 0.f;
    for (int s = lane; s < S; s += 64) {
        const float ms = Mr[s];
        if (ms != -INFINITY) lloc += Lr[s] * __builtin_amdgcn_exp2f(ms - mstar);
    }
    float Lsum = wave_sum(lloc);
    if constexpr (Grouped) {
        if (Sg > 0) {                 // lg = 0: the sum above alone, bit for bit the instance without groups
            float gloc = 0.f;
            for (int s = lane; s < Sg; s += 64) {
                const float ms = Mgr[s];
                if (ms != -INFINITY) gloc += Lgr[s] * __builtin_amdgcn_exp2f(ms - mstar);
            }
            Lsum += wave_sum(gloc);
        }
    }
    const float L = Lsum + (sa == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sa - mstar));
    const float inv = 1.f / L;
    T* orow = reinterpret_cast<T*>(a.o.ptr + ((int64_t)b * a.o.sb + (int64_t)head * a.o.sh + (int64_t)(Ragged ? prow + t : t) * a.o.sn) * es);
    for (int d = lane; d < D; d += 64) {
        float acc = 0.f;
#pragma unroll 8
        for (int s = 0; s < S; ++s) {
            const float ms = Mr[s];
            if (ms != -INFINITY) acc = fmaf(Or[(int64_t)s * D + d], __builtin_amdgcn_exp2f(ms - mstar), acc);
        }
        if constexpr (Grouped) {
#pragma unroll 8
            for (int s = 0; s < Sg; ++s) {     // no branch in front of the loads: a round of them is in flight at once
                const float ms = Mgr[s];
                acc = fmaf(Ogr[(int64_t)s * D + d], ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - mstar), acc);
            }
        }
        orow[d] = from_f32<T>(acc * inv);
    }
}

// sfa_ring_commit_dyn / _rows: a = clamp(count, 0, n) accepted chunk tokens (per row with per-sequence state); tokens
// [max(0, a - Wc), a) go to ring slot (write_pos + t) mod Wc of the row's device state.  Reads the state only:
// ring_advance_kernel moves it on afterwards.
__global__ __launch_bounds__(256) void ring_commit_kernel(MultiArgs a, const int* count, int es) {
    commit_piece(a, (int64_t)blockIdx.x * 256 + threadIdx.x, es, count);
}

// sfa_ring_commit_path_dyn / _rows: the same with the j-th stored token taken from chunk row path[b][j] (a tree's
// accepted root-to-leaf path), so that tokens [max(0, a - Wc), a) of the path go to slot (write_pos + j) mod Wc
__global__ __launch_bounds__(256) void ring_commit_path_kernel(MultiArgs a, const int* count, int es) {
    commit_piece<true>(a, (int64_t)blockIdx.x * 256 + threadIdx.x, es, count);
}

// sfa_ring_commit_slots / sfa_ring_commit_path_slots: the two kernels above on the rings and states of slots[b]
template <bool Path>
__global__ __launch_bounds__(256) void ring_commit_slots_kernel(MultiArgs a, const int* count, int es) {
    commit_piece<Path, true>(a, (int64_t)blockIdx.x * 256 + threadIdx.x, es, count);
}

// sfa_ring_commit_path_ragged_slots: the path commit of a pack, item = (hk * T + packed row) * cpr + ch.  The call has
// no preparation launch: the thread finds its row's sequence i by the binary search of ragged_prep_kernel.  Its row is
// position j of the sequence: with acc = clamp(count[i], 0, n_i), positions [max(0, acc - Wc), acc) store packed row
// c0_i + clamp(path[c0_i + j], 0, n_i - 1) (row c0_i + j without a path) into ring slot (write_pos + j) mod Wc of slot
// slots[i] - the piece commit_piece<Path, true> stores for the sequence passed as a [1, Hkv, n_i, D] chunk.
// Q (store_piece): void, or the pack's 16-bit type when the ring is FP8 (es stays the pack's element size); KA: Kv8Args then
// Paged: KA ends in PageArgs, the slot goes to row slot mod P of its page, a slot on an unmapped page is dropped
template <typename Q = void, bool Paged = false, typename... KA>
__global__ __launch_bounds__(256) void ring_commit_ragged_kernel(MultiArgs a, RaggedArgs rg, const int* count, int es,
                                                                 KA... ka) {
    static_assert(tail_is<false, !std::is_void_v<Q>, Paged, KA...>,
                  "FP8 ring: (..., Kv8Args); paged ring: (..., PageArgs); paged FP8 ring: (..., Kv8Args, PageArgs)");
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cpr = a.D * es / 16;
    if (item >= (int64_t)a.Hkv * rg.T * cpr) return;
    const int ch = (int)(item % cpr);
    const int64_t rest = item / cpr;
    const int tp = (int)(rest % rg.T);
    const int hk = (int)(rest / rg.T);
    int lo = 0, hi = rg.n_seq - 1;           // the last sequence that starts at or before the row
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ragged_seq(rg, mid).c0 <= tp) lo = mid;
        else hi = mid - 1;
    }
    const RaggedSeq s = ragged_seq(rg, lo);
    const int j = tp - s.c0;
    if (j < 0 || j >= s.n) return;           // a row no sequence covers
    const int c = cache_row<true>(a, lo);
    if (c < 0) return;
    const int last = clamp_count(count + lo, s.n);
    if (j >= last || j < last - a.wc) return;
    int slot = (int)(((int64_t)state_wp(a, c) + j) % a.wc);
    int drow = c;                // the ring's row of its buffer: the cache row, or the slot's page
    if constexpr (Paged) {
        const PageArgs& pg = arg_of<PageArgs>(ka...);
        if ((drow = page_at(pg, c, slot)) < 0) return;
        slot = page_row(pg, slot);
    }
    int src = j;
    if (a.path) {
        src = a.path[s.c0 + j];
        src = src < 0 ? 0 : (src >= s.n ? s.n - 1 : src);
    }
    const int64_t so = (int64_t)ch * 16, row = (int64_t)s.c0 + src, dso = piece_off<Q>(ch);
    const int ed = piece_es<Q>(es);
    const char* ks = a.kn.ptr + ((int64_t)hk * a.kn.sh + row * a.kn.sn) * es + so;
    const char* vs = a.vn.ptr + ((int64_t)hk * a.vn.sh + row * a.vn.sn) * es + so;
    char* kd = a.wk.ptr + ((int64_t)drow * a.wk.sb + (int64_t)hk * a.wk.sh + (int64_t)slot * a.wk.sn) * ed + dso;
    char* vd = a.wv.ptr + ((int64_t)drow * a.wv.sb + (int64_t)hk * a.wv.sh + (int64_t)slot * a.wv.sn) * ed + dso;
    store_piece<Q>(kd, vd, ks, vs, arg_of<Kv8Args>(ka...), a.Hkv, hk);
}

// sfa_ring_fill_varlen: the prefill placement of SinkCacheLayer._prefill for every sequence of a packed [1, Hkv, T, D]
// K/V, one 16-byte piece per thread.  item = ((b * Hkv + hk) * (ns + Wc) + j) * cpr + ch: j < ns is sink row j, j >= ns
// ring slot s = j - ns.  Sequence b = rows [cu[b], cu[b + 1]) of length L (offsets clamped into [0, T], so that bad
// offsets cannot address outside the pack) is placed by fill_place / fill_src: sink row j <- token j for j < sl =
// min(L, ns); with rest = L - sl, slot s <- token sl + s for s < rest when rest <= Wc, else token L - Wc + s (the newest
// Wc, wrapped at slot 0).  Rows and slots the sequence does not reach keep their content.  The first piece of each
// sequence writes its state row (fill_state): {sl, min(rest, Wc), rest < Wc ? rest : 0, L}.
// Slots (sfa_ring_fill_varlen_slots): sequence b goes to cache row and state row slots[b] of a pool of npool rows (a
// value outside [0, npool): the sequence is skipped); every other row of the pool keeps buffers and state.
// Q (store_piece): void, or the pack's 16-bit type when the pool is FP8 (cpr and es stay those of the pack); KA: Kv8Args then
// Paged (Slots): KA ends in PageArgs; wc = stride * P, ring slot s goes to row s mod P of its page, a slot on an
// unmapped page is dropped (the state row is written all the same)
template <bool Slots, typename Q = void, bool Paged = false, typename... KA>
__global__ __launch_bounds__(256) void ring_fill_varlen_kernel(View sk, View sv, View wk, View wv, View k, View v,
                                                               const int* cu, int* state, int n_seq, int Hkv, int ns,
                                                               int wc, int T, int cpr, int es, const int* slots,
                                                               int npool, KA... ka) {
    static_assert(tail_is<false, !std::is_void_v<Q>, Paged, KA...> && !(Paged && !Slots),
                  "FP8 pool: (..., Kv8Args); paged pool: (..., PageArgs); paged FP8 pool: (..., Kv8Args, PageArgs)");
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nj = ns + wc;
    if (item >= (int64_t)n_seq * Hkv * nj * cpr) return;
    const int ch = (int)(item % cpr);
    int64_t rest = item / cpr;
    const int j = (int)(rest % nj);
    rest /= nj;
    const int hk = (int)(rest % Hkv);
    const int b = (int)(rest / Hkv);
    int c = b;                   // the cache row
    if constexpr (Slots) {
        c = slots[b];
        if ((unsigned)c >= (unsigned)npool) return;
    }
    const RaggedSeq seq = ragged_seq(RaggedArgs{cu, nullptr, nullptr, n_seq, T, 0}, b);
    const int c0 = seq.c0;
    const FillPlace p = fill_place(seq.n, ns, wc);
    if (hk == 0 && j == 0 && ch == 0) fill_state(p, state + (int64_t)c * 4);
    const int src = fill_src(p, j);   // token index within the sequence, -1: nothing to store
    if (src < 0) return;
    const View *dk = j < ns ? &sk : &wk, *dv = j < ns ? &sv : &wv;
    int row = j < ns ? j : j - ns;
    int drow = c;                // the destination's row of its buffer: the cache row, or the page of a ring slot
    if constexpr (Paged) {
        if (j >= ns) {
            const PageArgs& pg = arg_of<PageArgs>(ka...);
            if ((drow = page_at(pg, c, row)) < 0) return;
            row = page_row(pg, row);
        }
    }
    const int64_t so = (int64_t)ch * 16, tok = (int64_t)c0 + src, dso = piece_off<Q>(ch);
    const int ed = piece_es<Q>(es);
    const char* ks = k.ptr + ((int64_t)hk * k.sh + tok * k.sn) * es + so;
    const char* vs = v.ptr + ((int64_t)hk * v.sh + tok * v.sn) * es + so;
    char* kd = dk->ptr + ((int64_t)drow * dk->sb + (int64_t)hk * dk->sh + (int64_t)row * dk->sn) * ed + dso;
    char* vd = dv->ptr + ((int64_t)drow * dv->sb + (int64_t)hk * dv->sh + (int64_t)row * dv->sn) * ed + dso;
    store_piece<Q>(kd, vd, ks, vs, arg_of<Kv8Args>(ka...), Hkv, hk);
}

// sfa_ring_copy_slots: pair i copies slot s = src_slots[i] of the source pool into slot d = dst_slots[i] of the
// destination pool (the same pool: a fork).  What the readers of s would read is copied in place: sink rows
// [0, sink_len) and ring slots [0, window_len), both clamped into the buffers as get_fill clamps them, and the state row
// verbatim (4 ints).  Every live row keeps its position, so write_pos means in d what it means in s; rows beyond the fill
// keep what d held.  A pair with s or d outside its pool, or with s == d in one pool (`same`), moves nothing.
// A workgroup is (pair, KV head, block of 256 * kCopyPieces consecutive 16-byte pieces of the live rows of that head:
// piece p = row * cpr + ch, row < sink_len a sink row, else ring slot row - sink_len); the grid covers the capacity
// (nblk blocks per head), blocks past the live pieces leave after the state read.  A thread first issues its
// kCopyPieces loads of K and of V, 256 pieces apart (a wave-instruction reads 1 KiB contiguous), without a branch among
// them, then stores: 2 * kCopyPieces independent 16-byte loads are in flight per thread.  The first thread of a pair's
// first block writes the state row; no workgroup of the launch reads that row (it is not a source: the aliasing rule of
// include/sfa.h).  -DSFA_COPY_PIECES=n: development builds for tools/kbench_fork.py.
#ifndef SFA_COPY_PIECES
#define SFA_COPY_PIECES 4
#endif
constexpr int kCopyPieces = SFA_COPY_PIECES;

struct CopyPools {
    View sk, sv, wk, wv;
    int* state;
    const int* slots;
    int S;
};

// Paged (sfa_ring_copy_paged_slots): PA = (PageArgs of the source, PageArgs of the destination); wc = stride * P of
// both.  Ring slot j is read from row j mod P of its source page (an unmapped one: page 0) and stored into row j mod P
// of its destination page (an unmapped one: the piece is dropped).  Sink rows and the state row as above.
template <bool Paged = false, typename... PA>
__global__ __launch_bounds__(256) void ring_copy_slots_kernel(CopyPools src, CopyPools dst, int Hkv, int ns, int wc,
                                                              int cpr, int es, int nblk, int same, PA... pa) {
    static_assert(sizeof...(PA) == (Paged ? 2 : 0), "paged pools: (..., PageArgs src, PageArgs dst)");
    const int blk = (int)(blockIdx.x % (unsigned)nblk);
    const int rest = (int)(blockIdx.x / (unsigned)nblk);
    const int hk = rest % Hkv, pair = rest / Hkv;
    const int s = src.slots[pair], d = dst.slots[pair];
    if ((unsigned)s >= (unsigned)src.S || (unsigned)d >= (unsigned)dst.S || (same && s == d)) return;
    const int* st = src.state + (int64_t)s * 4;
    const int st0 = st[0], st1 = st[1], st2 = st[2], st3 = st[3];
    const int sl = st0 < 0 ? 0 : (st0 > ns ? ns : st0);
    const int wl = st1 < 0 ? 0 : (st1 > wc ? wc : st1);
    if (blk == 0 && hk == 0 && threadIdx.x == 0) {
        int* dt = dst.state + (int64_t)d * 4;
        dt[0] = st0, dt[1] = st1, dt[2] = st2, dt[3] = st3;
    }
    const int live = (sl + wl) * cpr;            // < 2^30: checked on the host at the capacity
    const int p0 = blk * (256 * kCopyPieces);
    if (p0 >= live) return;
    // the 16 bytes of piece (r, c) in the K (v = false) or V buffer of a pool; slot: the pair's slot of that pool
    // Paged: `slot` of a ring row is its page instead (pages_of below), the row its place in the page
    [[maybe_unused]] PageArgs spg{}, dpg{};
    if constexpr (Paged) {
        const PageArgs both[2] = {pa...};
        spg = both[0], dpg = both[1];
    }
    auto at = [&](const CopyPools& pl, int slot, int r, int c, bool v) {
        const bool sink = r < sl;
        const View& b = sink ? (v ? pl.sv : pl.sk) : (v ? pl.wv : pl.wk);
        int64_t rr = sink ? r : r - sl;
        if constexpr (Paged) rr = sink ? rr : page_row(spg, (int)rr);      // one P for both pools
        return reinterpret_cast<u32x4*>(b.ptr + ((int64_t)slot * b.sb + (int64_t)hk * b.sh + rr * b.sn) * es + (int64_t)c * 16);
    };
    // paged pools: the buffer row of piece row r in the source (the slot for a sink row, else the page; unmapped: page 0)
    // and in the destination (unmapped: -1, the piece is not stored)
    [[maybe_unused]] auto pages_of = [&](int r, int& srow, int& drow) {
        srow = s, drow = d;
        if constexpr (Paged) {
            if (r >= sl) {
                const int e = page_at(spg, s, r - sl);
                srow = e < 0 ? 0 : e;
                drow = page_at(dpg, d, r - sl);
            }
        }
    };
    // The thread's pieces p0 + tid + 256 u as (row, chunk): one division, then steps of 256 pieces.  full (wave-uniform):
    // every piece of the block is live, and the loads and stores carry no predicate.  In the last block of a head a
    // piece past the live ones is loaded from the last live piece (a valid address) and not stored.
    auto copy = [&](auto full_block) {
        constexpr bool full = decltype(full_block)::value;
        int row[kCopyPieces], ch[kCopyPieces];
        bool ok[kCopyPieces];
        const int p = p0 + (int)threadIdx.x, rstep = 256 / cpr, cstep = 256 - rstep * cpr;
        int r = p / cpr, c = p - r * cpr;
#pragma unroll
        for (int u = 0; u < kCopyPieces; ++u) {
            ok[u] = full || p + u * 256 < live;
            row[u] = ok[u] ? r : sl + wl - 1, ch[u] = ok[u] ? c : cpr - 1;
            r += rstep, c += cstep;
            if (c >= cpr) c -= cpr, ++r;
        }
        u32x4 kr[kCopyPieces], vr[kCopyPieces];
        if constexpr (Paged) {     // the table entries first (independent loads), then the pieces as below
            int sr[kCopyPieces], dr[kCopyPieces];
#pragma unroll
            for (int u = 0; u < kCopyPieces; ++u) pages_of(row[u], sr[u], dr[u]);
#pragma unroll
            for (int u = 0; u < kCopyPieces; ++u)
                kr[u] = *at(src, sr[u], row[u], ch[u], false), vr[u] = *at(src, sr[u], row[u], ch[u], true);
#pragma unroll
            for (int u = 0; u < kCopyPieces; ++u)
                if (ok[u] && dr[u] >= 0) *at(dst, dr[u], row[u], ch[u], false) = kr[u], *at(dst, dr[u], row[u], ch[u], true) = vr[u];
            return;
        }
#pragma unroll
        for (int u = 0; u < kCopyPieces; ++u)
            kr[u] = *at(src, s, row[u], ch[u], false), vr[u] = *at(src, s, row[u], ch[u], true);
#pragma unroll
        for (int u = 0; u < kCopyPieces; ++u)
            if (ok[u]) *at(dst, d, row[u], ch[u], false) = kr[u], *at(dst, d, row[u], ch[u], true) = vr[u];
    };
    if (p0 + 256 * kCopyPieces <= live) copy(std::true_type{});
    else copy(std::false_type{});
}

// sfa_ring_export_slots: the inverse of ring_fill_varlen_kernel<true>.  Sequence i of the pack k_out / v_out
// [1, Hkv, T, D] owns the packed rows [c0, c0 + m) (cu clamped by ragged_seq) and names slot c = slots[i] with the state
// row {sl, wl, wp, seen}, clamped as get_fill clamps it.  Its live tokens in token order: index j < sl is sink row j at
// position j; index j = sl + r, r < wl, is ring slot (wp - wl + r) mod Wc at position seen - wl + r, the oldest ring
// token first (r while the ring fills, where wp == wl, and after a prefill, which leaves a full ring at wp == 0;
// (wp + r) mod Wc once commits have wrapped it).  Row j < min(m, sl + wl) gets token j; every other row of the pack - the
// tail of a sequence, a sequence whose slot is outside [0, S), a row that no sequence covers - is written as zeros, and
// pos gets the position of a token row and -1 of a zeroed one.  Nothing of the pool or the state is written.
// A workgroup is (KV head, block of 256 * kExportPieces consecutive 16-byte pieces of the head's T rows of the pack:
// piece p = row * cpr + ch), so the grid follows T and not the pool's capacity.  It finds the last sequence that starts at
// or before its first row by the binary search of ring_commit_ragged_kernel, on block-uniform values (scalar loads); when
// no later sequence starts inside the block, the sequence, its slot and the state row are read once for the workgroup.
// Otherwise each piece walks on from that sequence and reads its own.  As in ring_copy_slots_kernel a thread issues its
// kExportPieces loads of K and of V, 256 pieces apart, without a branch among them, before its first store; a piece with
// nothing to read loads the first bytes of the ring buffers (a valid address) and stores zeros.
// Q = void: the pack has the pool's dtype and 16 bytes are copied.  Q = the pack's 16-bit type, KA starts with Kv8Args: an
// FP8 pool, 8 codes are read and kv8_read makes the 16 bytes, as the packed step does on the way into LDS.
// Paged: KA ends in PageArgs; a ring slot is read from row slot mod P of its page (page_at), a slot on an unmapped page
// gives zeros and keeps its position in pos.
#ifndef SFA_EXPORT_PIECES
#define SFA_EXPORT_PIECES 4
#endif
constexpr int kExportPieces = SFA_EXPORT_PIECES;

struct ExportArgs {
    View sk, sv, wk, wv, ko, vo;
    const int* cu;
    const int* state;
    const int* slots;
    int* pos;                    // [T] or null
    int n_seq, S, Hkv, ns, wc, T, cpr, es, nblk;
};

// sequence i of an export: its packed rows [c0, c0 + m), its slot (-1: outside the pool) and that slot's clamped state
struct ExportSeq {
    int c0, m, c, sl, wl, wp, seen;
};

__device__ __forceinline__ int export_start(const ExportArgs& a, int i) {
    const int c = a.cu[i];
    return c < 0 ? 0 : (c > a.T ? a.T : c);
}

__device__ __forceinline__ ExportSeq export_seq(const ExportArgs& a, int i) {
    const RaggedSeq s = ragged_seq(RaggedArgs{a.cu, nullptr, nullptr, a.n_seq, a.T, 0, nullptr}, i);
    const int c = a.slots[i];
    const bool in = (unsigned)c < (unsigned)a.S;
    const int* st = a.state + (int64_t)(in ? c : 0) * 4;      // S >= 1: row 0 is a valid address
    const int sl = st[0], wl = st[1], wp = st[2], seen = st[3];
    return ExportSeq{s.c0, s.n, in ? c : -1, sl < 0 ? 0 : (sl > a.ns ? a.ns : sl), wl < 0 ? 0 : (wl > a.wc ? a.wc : wl),
                     wp < 0 ? 0 : (wp >= a.wc ? a.wc - 1 : wp), seen};
}

template <typename Q = void, bool Paged = false, typename... KA>
__global__ __launch_bounds__(256) void ring_export_slots_kernel(ExportArgs a, KA... ka) {
    constexpr bool KV8 = !std::is_void_v<Q>;
    static_assert(tail_is<false, KV8, Paged, KA...>,
                  "FP8 pool: (..., Kv8Args); paged pool: (..., PageArgs); paged FP8 pool: (..., Kv8Args, PageArgs)");
    using Raw = std::conditional_t<KV8, uint2, u32x4>;        // what a thread reads of one piece
    const int blk = (int)(blockIdx.x % (unsigned)a.nblk), hk = (int)(blockIdx.x / (unsigned)a.nblk);
    const int total = a.T * a.cpr;                   // < 2^30: checked on the host
    const int p0 = blk * (256 * kExportPieces);
    const int plast = p0 + 256 * kExportPieces <= total ? p0 + 256 * kExportPieces - 1 : total - 1;
    const int r0 = p0 / a.cpr, r1 = plast / a.cpr;
    int lo = 0, hi = a.n_seq - 1;                    // the last sequence that starts at or before row r0
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (export_start(a, mid) <= r0) lo = mid;
        else hi = mid - 1;
    }
    const bool one = lo + 1 >= a.n_seq || export_start(a, lo + 1) > r1;      // no later sequence starts in the block
    const ExportSeq e0 = export_seq(a, lo);
    [[maybe_unused]] float ksc = 1.f, vsc = 1.f;
    if constexpr (KV8) ksc = kv8_scale(arg_of<Kv8Args>(ka...), 0, a.Hkv, hk), vsc = kv8_scale(arg_of<Kv8Args>(ka...), 1, a.Hkv, hk);
    const int esrc = KV8 ? 1 : a.es, sbytes = KV8 ? 8 : 16;
    auto run = [&](auto one_seq) {
        constexpr bool uni = decltype(one_seq)::value;
        const int p = p0 + (int)threadIdx.x, rstep = 256 / a.cpr, cstep = 256 - rstep * a.cpr;
        int r = p / a.cpr, c = p - r * a.cpr;
        [[maybe_unused]] int seq = lo;
        const char *ks[kExportPieces], *vs[kExportPieces];
        int64_t doff_k[kExportPieces], doff_v[kExportPieces];
        int pos[kExportPieces], row[kExportPieces];
        bool in[kExportPieces], data[kExportPieces], first[kExportPieces];
#pragma unroll
        for (int u = 0; u < kExportPieces; ++u) {
            in[u] = p + u * 256 < total;
            const int rr = in[u] ? r : a.T - 1, cc = in[u] ? c : a.cpr - 1;
            ExportSeq e = e0;
            if constexpr (!uni) {
                while (seq + 1 < a.n_seq && export_start(a, seq + 1) <= rr) ++seq;
                e = export_seq(a, seq);
            }
            const int j = rr - e.c0, live = e.sl + e.wl;
            const bool tok = e.c >= 0 && j >= 0 && j < (e.m < live ? e.m : live);
            const bool sink = tok && j < e.sl;
            const int rg = j - e.sl;
            int slot = !tok ? 0 : sink ? j : (int)(((int64_t)e.wp - e.wl + rg + a.wc) % a.wc);
            int brow = tok ? e.c : 0;            // the source's row of its buffer: the cache row, or the page of a ring slot
            bool mapped = true;
            if constexpr (Paged) {
                if (!sink) {
                    const PageArgs& pg = arg_of<PageArgs>(ka...);
                    const int e_pg = page_at(pg, brow, slot);
                    mapped = e_pg >= 0;
                    brow = mapped ? e_pg : 0, slot = page_row(pg, slot);
                }
            }
            const View &bk = sink ? a.sk : a.wk, &bv = sink ? a.sv : a.wv;
            ks[u] = bk.ptr + ((int64_t)brow * bk.sb + (int64_t)hk * bk.sh + (int64_t)slot * bk.sn) * esrc + (int64_t)cc * sbytes;
            vs[u] = bv.ptr + ((int64_t)brow * bv.sb + (int64_t)hk * bv.sh + (int64_t)slot * bv.sn) * esrc + (int64_t)cc * sbytes;
            doff_k[u] = ((int64_t)hk * a.ko.sh + (int64_t)rr * a.ko.sn) * a.es + (int64_t)cc * 16;
            doff_v[u] = ((int64_t)hk * a.vo.sh + (int64_t)rr * a.vo.sn) * a.es + (int64_t)cc * 16;
            pos[u] = !tok ? -1 : sink ? j : e.seen - e.wl + rg;
            row[u] = rr, data[u] = tok && mapped, first[u] = in[u] && cc == 0;
            r += rstep, c += cstep;
            if (c >= a.cpr) c -= a.cpr, ++r;
        }
        Raw kr[kExportPieces], vr[kExportPieces];
#pragma unroll
        for (int u = 0; u < kExportPieces; ++u)
            kr[u] = *reinterpret_cast<const Raw*>(ks[u]), vr[u] = *reinterpret_cast<const Raw*>(vs[u]);
#pragma unroll
        for (int u = 0; u < kExportPieces; ++u) {
            u32x4 ko, vo;
            if constexpr (KV8) ko = kv8_read<Q, true>(kr[u].x, kr[u].y, ksc), vo = kv8_read<Q, true>(vr[u].x, vr[u].y, vsc);
            else ko = kr[u], vo = vr[u];
            const u32x4 zero = {0u, 0u, 0u, 0u};
            if (in[u]) {
                *reinterpret_cast<u32x4*>(a.ko.ptr + doff_k[u]) = data[u] ? ko : zero;
                *reinterpret_cast<u32x4*>(a.vo.ptr + doff_v[u]) = data[u] ? vo : zero;
            }
            if (a.pos && hk == 0 && first[u]) a.pos[row[u]] = pos[u];
        }
    };
    if (one) run(std::true_type{});
    else run(std::false_type{});
}

// sfa_ring_share_paged_slots: the unpaged half of a fork whose ring pages are shared through the table.  Pair i copies the
// live sink rows (j < clamp(sink_len, 0, num_sink)) and the state row of slot s into slot d with the skip rules of
// ring_copy_slots_kernel; src / dst carry no ring views, no ring byte is read or written.  A workgroup is (pair, KV head,
// block of 256 16-byte pieces of that head's sink rows); the first thread of a pair's first block writes the state row.
__global__ __launch_bounds__(256) void ring_share_slots_kernel(CopyPools src, CopyPools dst, int Hkv, int ns, int cpr,
                                                               int es, int nblk, int same) {
    const int blk = (int)(blockIdx.x % (unsigned)nblk);
    const int rest = (int)(blockIdx.x / (unsigned)nblk);
    const int hk = rest % Hkv, pair = rest / Hkv;
    const int s = src.slots[pair], d = dst.slots[pair];
    if ((unsigned)s >= (unsigned)src.S || (unsigned)d >= (unsigned)dst.S || (same && s == d)) return;
    const int* st = src.state + (int64_t)s * 4;
    const int st0 = st[0], st1 = st[1], st2 = st[2], st3 = st[3];
    const int sl = st0 < 0 ? 0 : (st0 > ns ? ns : st0);
    if (blk == 0 && hk == 0 && threadIdx.x == 0) {
        int* dt = dst.state + (int64_t)d * 4;
        dt[0] = st0, dt[1] = st1, dt[2] = st2, dt[3] = st3;
    }
    const int p = blk * 256 + (int)threadIdx.x;
    if (p >= sl * cpr) return;
    const int r = p / cpr, c = p - r * cpr;
    auto at = [&](const View& b, int slot) {
        return reinterpret_cast<u32x4*>(b.ptr + ((int64_t)slot * b.sb + (int64_t)hk * b.sh + (int64_t)r * b.sn) * es + (int64_t)c * 16);
    };
    const u32x4 kr = *at(src.sk, s), vr = *at(src.sv, s);
    *at(dst.sk, d) = kr, *at(dst.sv, d) = vr;
}

// sfa_pages_copy: pair i copies the whole page s = src_pages[i] onto page d = dst_pages[i] of the page buffers
// wk / wv [n_pages, Hkv, P, D], K and V, as bytes (the copy-on-write of a shared page).  A pair with s or d outside
// [0, n_pages) or with s == d moves nothing.  A workgroup is (pair, block of 256 * kPagePieces consecutive 16-byte pieces
// of the page: piece p = (hk * P + row) * cpr + ch); it reads the pair's two page ids once (blockIdx only: scalar loads).
// As in ring_copy_slots_kernel a thread issues its kPagePieces loads of K and of V, 256 pieces apart (a wave-instruction
// reads 1 KiB contiguous within a row run), before its first store; a piece past the page in the last block is loaded
// from the page's last piece (a valid address) and not stored.  Page, head and row offsets are 64-bit products of the
// view's strides, so the buffers may be strided views and lie behind 4 GiB.
constexpr int kPagePieces = 4;

__global__ __launch_bounds__(256) void pages_copy_kernel(View wk, View wv, const int* src_pages, const int* dst_pages,
                                                         int n_pages, int P, int cpr, int es, int nblk, int per_page) {
    const int blk = (int)(blockIdx.x % (unsigned)nblk), pair = (int)(blockIdx.x / (unsigned)nblk);
    const int s = src_pages[pair], d = dst_pages[pair];
    if ((unsigned)s >= (unsigned)n_pages || (unsigned)d >= (unsigned)n_pages || s == d) return;
    const int p = blk * (256 * kPagePieces) + (int)threadIdx.x;     // < per_page + 1024 < 2^31 (host check)
    const int rstep = 256 / cpr, cstep = 256 - rstep * cpr;
    int r = p / cpr, c = p - r * cpr;            // r = hk * P + row
    int64_t off_k[kPagePieces], off_v[kPagePieces];
    bool ok[kPagePieces];
#pragma unroll
    for (int u = 0; u < kPagePieces; ++u) {
        ok[u] = p + u * 256 < per_page;
        const int rr = ok[u] ? r : per_page / cpr - 1, cc = ok[u] ? c : cpr - 1;
        const int hk = rr / P, row = rr - hk * P;
        off_k[u] = ((int64_t)hk * wk.sh + (int64_t)row * wk.sn) * es + (int64_t)cc * 16;
        off_v[u] = ((int64_t)hk * wv.sh + (int64_t)row * wv.sn) * es + (int64_t)cc * 16;
        r += rstep, c += cstep;
        if (c >= cpr) c -= cpr, ++r;
    }
    const char *ks = wk.ptr + (int64_t)s * wk.sb * es, *vs = wv.ptr + (int64_t)s * wv.sb * es;
    char *kd = wk.ptr + (int64_t)d * wk.sb * es, *vd = wv.ptr + (int64_t)d * wv.sb * es;
    u32x4 kr[kPagePieces], vr[kPagePieces];
#pragma unroll
    for (int u = 0; u < kPagePieces; ++u)
        kr[u] = *reinterpret_cast<const u32x4*>(ks + off_k[u]), vr[u] = *reinterpret_cast<const u32x4*>(vs + off_v[u]);
#pragma unroll
    for (int u = 0; u < kPagePieces; ++u)
        if (ok[u]) *reinterpret_cast<u32x4*>(kd + off_k[u]) = kr[u], *reinterpret_cast<u32x4*>(vd + off_v[u]) = vr[u];
}

// one state row after every reader of it: write_pos += acc (mod Wc), window_len = min(window_len + acc, Wc), and - for a
// per-sequence row - seen += acc.  Plain stores from vector lanes.
__device__ __forceinline__ void advance_row(int* st, int acc, int wc, bool seen) {
    int wl = st[1], wp = st[2];
    wl = wl < 0 ? 0 : (wl > wc ? wc : wl);
    wp = wp < 0 ? 0 : (wp >= wc ? wc - 1 : wp);
    st[1] = wl + acc < wc ? wl + acc : wc;
    st[2] = (int)(((int64_t)wp + acc) % wc);
    if (seen) st[3] += acc;
}

// one thread per state row (`rows` of them, stride `stride`: 0 = the shared state, 4 = per-sequence rows with count
// [rows]): advance by clamp(count, 0, n), all n without a count
__global__ void ring_advance_kernel(int* state, const int* count, int n, int wc, int rows, int stride) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= rows) return;
    advance_row(state + (int64_t)r * stride, count ? clamp_count(count + (stride ? r : 0), n) : n, wc, stride != 0);
}

// the same for a slot call: thread r advances state row slots[r]; an inactive row moves nothing
__global__ void ring_advance_slots_kernel(int* state, const int* count, int n, int wc, int rows, const int* slots,
                                          int npool) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= rows) return;
    const int c = slots[r];
    if ((unsigned)c >= (unsigned)npool) return;
    advance_row(state + (int64_t)c * 4, count ? clamp_count(count + r, n) : n, wc, true);
}

// the same for a packed call: thread r advances state row slots[r] by n_r = the length of sequence r; an inactive or
// empty sequence moves nothing.  An admitting sequence (flag, seen == 0: this launch is the first writer of the row)
// gets the state of its prefill placement.  commit_seq (per-sequence commit): a sequence whose entry is 0 moves nothing.
// count (sfa_ring_commit_path_ragged_slots): by clamp(count[r], 0, n_r) in place of n_r.
__global__ void ring_advance_ragged_kernel(int* state, RaggedArgs rg, int ns, int wc, const int* slots, int npool,
                                           const int* count) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= rg.n_seq) return;
    const int c = slots[r];
    if ((unsigned)c >= (unsigned)npool) return;
    if (rg.commit_seq && !rg.commit_seq[r]) return;
    const int n = ragged_seq(rg, r).n;
    const int acc = count ? clamp_count(count + r, n) : n;
    if (!acc) return;
    int* st = state + (int64_t)c * 4;
    if (admits(rg.admit, st)) fill_state(fill_place(acc, ns, wc), st);
    else advance_row(st, acc, wc, true);
}

// advance every state row after the launches that read it (shared state: one row); rg: by the lengths of a pack
int launch_advance(const MultiArgs& a, const int* count, const RaggedArgs* rg, hipStream_t stream) {
    int* state = const_cast<int*>(a.state);
    const int nrow = rg ? rg->n_seq : a.sstride ? a.B : 1;
    if (nrow <= 0) return SFA_OK;
    const dim3 grid((unsigned)cdiv64(nrow, 256)), block(nrow < 256 ? nrow : 256);
    if (rg) {
        ring_advance_ragged_kernel<<<grid, block, 0, stream>>>(state, *rg, a.ns, a.wc, a.slots, a.npool, count);
        return launch_status("ring_advance_ragged");
    }
    if (a.slots) {
        ring_advance_slots_kernel<<<grid, block, 0, stream>>>(state, count, a.n, a.wc, nrow, a.slots, a.npool);
        return launch_status("ring_advance_slots");
    }
    ring_advance_kernel<<<grid, block, 0, stream>>>(state, count, a.n, a.wc, nrow, a.sstride);
    return launch_status("ring_advance");
}

constexpr int64_t kTargetWgs = 2048;

int64_t want_splits(int64_t B, int64_t Hkv, int64_t nrb) {
    const int64_t base = B * Hkv * nrb > 0 ? B * Hkv * nrb : 1;
    const int64_t w = cdiv64(kTargetWgs, base);
    return w < 1 ? 1 : w;
}

// largest split count any cache state with at most Nkv keys (sink + ring + chunk) plans: the tiles of three segments
// number at most ceil(Nkv / 32) + 2
int64_t max_splits(int64_t B, int64_t Hkv, int64_t nrb, int64_t Nkv) {
    int64_t s = cdiv64(cdiv64(Nkv, kTile) + 2, kMinTiles);
    const int64_t w = want_splits(B, Hkv, nrb);
    if (s > w) s = w;
    return s < 1 ? 1 : s;
}

bool mfma_head_dim(int D) { return D == 64 || D == 80 || D == 96 || D == 128; }

// The kernel instances that exist, one line per mode of a call: f gets the (Dyn, Tree, Slots, Ragged) of the split
// kernels (the reduce kernel has no Tree).  A new mode is a new field of RingCall / MultiArgs plus one line here.
template <bool Dyn_, bool Tree_, bool Slots_, bool Ragged_>
struct Mode {
    static constexpr bool Dyn = Dyn_, Tree = Tree_, Slots = Slots_, Ragged = Ragged_;
};

template <typename F>
void dispatch_mode(const MultiArgs& a, const RaggedArgs* rg, F&& f) {
    if (rg && a.parent) f(Mode<true, true, true, true>{});                        // packed: slots and device rows
    else if (rg) f(Mode<true, false, true, true>{});
    else if (a.slots && a.parent) f(Mode<true, true, true, false>{});             // slot calls: device rows
    else if (a.slots) f(Mode<true, false, true, false>{});
    else if (a.state && a.parent) f(Mode<true, true, false, false>{});
    else if (a.state) f(Mode<true, false, false, false>{});
    else if (a.parent) f(Mode<false, true, false, false>{});
    else f(Mode<false, false, false, false>{});
}

// the table argument of a paged pool (pt.table set): the API has checked that P is a power of two
PageArgs page_args(const PageTable& pt) {
    int shift = 0;
    while ((1ll << shift) < pt.page_size) ++shift;
    return PageArgs{pt.table, (int)pt.stride, shift, (int)pt.n_pages};
}

// The pool forms of the instances, one line per kind of pool: f gets the (KV8, Paged) of the kernels that read a pool and
// the Q of the ones that store into it (void: the rows are copied; FP8: the 16-bit type `act_dtype` of the activations,
// which are quantised - a launcher of kernels that only read the pool leaves it out), then the trailing arguments of
// that form: none, (Kv8Args), (PageArgs) or (Kv8Args, PageArgs).  A further kind of pool is a field of SlotPool, its
// kernel argument and its lines here.
template <typename Q_, bool Paged_>
struct PoolForm {
    using Q = Q_;
    static constexpr bool KV8 = !std::is_void_v<Q_>, Paged = Paged_;
};

template <typename F>
void dispatch_pool(const SlotPool& pool, F&& f, int act_dtype = SFA_DTYPE_BF16) {
    const Kv8Args kv{pool.kv_scale};
    const bool f16 = act_dtype == SFA_DTYPE_F16;
    if (!pool.fp8 && !pool.pt.table) f(PoolForm<void, false>{});
    else if (!pool.fp8) f(PoolForm<void, true>{}, page_args(pool.pt));
    else if (!pool.pt.table) f16 ? f(PoolForm<f16_t, false>{}, kv) : f(PoolForm<bf16_t, false>{}, kv);
    else f16 ? f(PoolForm<f16_t, true>{}, kv, page_args(pool.pt)) : f(PoolForm<bf16_t, true>{}, kv, page_args(pool.pt));
}

// the tail of sfa_last_path that names the pool
const char* pool_tag(const SlotPool& pool) {
    return pool.fp8 ? (pool.pt.table ? "_paged_kvfp8" : "_kvfp8") : pool.pt.table ? "_paged" : "";
}

// launch_status of a split launch: decode_{multi,tree}_{mfma,f32}[_slots | _ragged]
int split_status(const MultiArgs& a, const RaggedArgs* rg, const char* kind) {
    char tag[40];
    snprintf(tag, sizeof(tag), "decode_%s_%s%s", a.parent ? "tree" : "multi", kind, rg ? "_ragged" : a.slots ? "_slots" : "");
    return launch_status(tag);
}

// pool (packed calls only): the (Dyn, Slots, Ragged) instances in the form of the pool, Tree on or off
// grp (a grouped call: paged pool, no tree): the grouped instance of that form, its shared-phase block ids in front
template <typename T, int D>
int launch_mfma(const MultiArgs& a, const RaggedArgs* rg, const SlotPool& pool, const GroupArgs* grp, hipStream_t stream) {
    const dim3 grid((unsigned)((int64_t)a.B * a.Hkv * a.Sw * a.nrb + (grp ? grp->nsh : 0)));
    dispatch_mode(a, rg, [&](auto m) {
        using M = decltype(m);
        if constexpr (M::Ragged)
            dispatch_pool(pool, [&](auto p, auto... tail) {
                using P = decltype(p);
                if constexpr (P::Paged && !M::Tree) {
                    if (grp) {
                        multi_split_mfma_kernel<T, D, M::Dyn, false, M::Slots, true, P::KV8, true><<<grid, kWaves * 64, 0, stream>>>(a, *rg, tail..., *grp);
                        return;
                    }
                }
                multi_split_mfma_kernel<T, D, M::Dyn, M::Tree, M::Slots, true, P::KV8, P::Paged><<<grid, kWaves * 64, 0, stream>>>(a, *rg, tail...);
            });
        else multi_split_mfma_kernel<T, D, M::Dyn, M::Tree, M::Slots><<<grid, kWaves * 64, 0, stream>>>(a);
    });
    return split_status(a, rg, "mfma");
}

template <typename T>
int launch_mfma_d(const MultiArgs& a, const RaggedArgs* rg, const SlotPool& pool, const GroupArgs* grp, hipStream_t stream) {
    switch (a.D) {
        case 64: return launch_mfma<T, 64>(a, rg, pool, grp, stream);
        case 80: return launch_mfma<T, 80>(a, rg, pool, grp, stream);
        case 96: return launch_mfma<T, 96>(a, rg, pool, grp, stream);
        case 128: return launch_mfma<T, 128>(a, rg, pool, grp, stream);
    }
    set_error("decode_multi: no MFMA kernel for head dim %d", a.D);
    return SFA_ERR_UNSUPPORTED;
}

// split launch, reduce (+ commit) launch, state advance; rg: the packed call (a.B = 1, a.n = T, a.R = G * T)
// pool: that of a packed call (the API admits an FP8 or paged one for the MFMA instances only)
template <typename T>
int launch_rest(const MultiArgs& a, const RaggedArgs* rg, const SlotPool& pool, const GroupArgs* grp, bool mfma, hipStream_t stream) {
    int st = SFA_OK;
    const int64_t rows = (int64_t)a.B * a.Hkv * a.R;
    if constexpr (sizeof(T) == 2) st = mfma ? launch_mfma_d<T>(a, rg, pool, grp, stream) : SFA_OK;
    if (!mfma) {
        const dim3 grid((unsigned)cdiv64(rows, 4), (unsigned)a.Sw);
        dispatch_mode(a, rg, [&](auto m) {
            using M = decltype(m);
            if constexpr (M::Ragged) multi_split_f32_kernel<T, M::Dyn, M::Tree, M::Slots, true><<<grid, 256, 0, stream>>>(a, *rg);
            else multi_split_f32_kernel<T, M::Dyn, M::Tree, M::Slots><<<grid, 256, 0, stream>>>(a);
        });
        st = split_status(a, rg, "f32");
    }
    if (st) return st;
    const int nred = (int)cdiv64(rows, 4);
    int64_t ncommit = 0;
    if (a.commit) {      // 16-byte pieces of the stored tokens AS THEY ARE READ (T's, whatever the pool stores): every row of a pack, else the last min(n, Wc) of the chunk
        const int64_t ncm = rg || a.n < a.wc ? a.n : a.wc;
        ncommit = cdiv64((int64_t)a.B * a.Hkv * ncm * (a.D * (int64_t)sizeof(T) / 16), 256);
    }
    const dim3 rgrid((unsigned)(nred + ncommit));
    dispatch_mode(a, rg, [&](auto m) {
        using M = decltype(m);
        if constexpr (M::Ragged && sizeof(T) == 2)
            dispatch_pool(pool, [&](auto p, auto... tail) {
                using P = decltype(p);
                if constexpr (P::Paged) {
                    if (grp) {
                        multi_reduce_kernel<T, M::Dyn, M::Slots, true, P::KV8, true><<<rgrid, 256, 0, stream>>>(a, nred, *rg, tail..., *grp);
                        return;
                    }
                }
                multi_reduce_kernel<T, M::Dyn, M::Slots, true, P::KV8, P::Paged><<<rgrid, 256, 0, stream>>>(a, nred, *rg, tail...);
            });
        else if constexpr (M::Ragged) multi_reduce_kernel<T, M::Dyn, M::Slots, true><<<rgrid, 256, 0, stream>>>(a, nred, *rg);
        else multi_reduce_kernel<T, M::Dyn, M::Slots><<<rgrid, 256, 0, stream>>>(a, nred);
    });
    if ((st = launch_status(rg ? "decode_multi_reduce_ragged" : "decode_multi_reduce"))) return st;
    if (a.state && a.commit)     // every reader of the state has finished: advance it (each row) by n (its n_i)
        st = launch_advance(a, nullptr, rg, stream);
    return st;
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// The kernel argument of a call, filled from the descriptor in this one place.  The commit launcher (attend = false)
// takes the ring, the chunk, the state and the path / slots and leaves the rest zero; an attention launcher adds its
// plan (want, T0 .. S, Sw) and the partials (Mp, Lp, Op) itself.
MultiArgs multi_args(const RingCall& c, bool attend) {
    MultiArgs a{};
    a.wk = make_view(c.window_k), a.wv = make_view(c.window_v), a.kn = make_view(c.k_new), a.vn = make_view(c.v_new);
    a.B = (int)c.k_new->shape[0], a.Hkv = (int)c.k_new->shape[1], a.n = (int)c.k_new->shape[2], a.D = (int)c.k_new->shape[3];
    a.wc = (int)c.window_k->shape[2];
    a.state = c.state, a.sstride = c.mode == RingState::Rows ? 4 : 0;
    a.path = c.path, a.pathstride = (int)c.path_bstride;
    a.slots = c.slots, a.npool = (int)c.window_k->shape[0];
    if (!attend) return a;
    a.q = make_view(c.q), a.sk = make_view(c.sink_k), a.sv = make_view(c.sink_v), a.o = make_view(c.o);
    a.s_aux = c.s_aux;
    a.G = (int)(c.q->shape[1] / c.k_new->shape[1]);
    a.R = a.G * a.n;
    a.nrb = (int)cdiv64(a.R, 32);
    a.sink_len = (int)c.sink_len, a.wl = (int)c.window_len, a.wp = (int)c.write_pos;
    a.ns = (int)c.sink_k->shape[2];
    a.scale_log2 = c.scale * kLog2e;
    a.commit = c.commit ? 1 : 0;
    a.parent = c.parent, a.pstride = (int)c.parent_bstride;
    return a;
}

// the launches of an attention call by q's dtype; *mfma: whether the MFMA split kernel serves it
int launch_dtype(const RingCall& c, const MultiArgs& a, const RaggedArgs* rg, bool* mfma, const char** dname,
                 const GroupArgs* grp = nullptr) {
    const int dt = c.q->dtype;
    *mfma = dt != SFA_DTYPE_F32 && mfma_head_dim(a.D) && !(c.flags & SFA_FLAG_FORCE_GENERIC);
    *dname = dt == SFA_DTYPE_F32 ? "f32" : dt == SFA_DTYPE_F16 ? "f16" : "bf16";
    if ((c.pool.fp8 || c.pool.pt.table) && !*mfma) {    // refused by the API before: no f32-accumulate instance reads an FP8 or a paged pool
        set_error("decode_ragged%s%s: no kernel instance for this call", c.pool.pt.table ? "_paged" : "", c.pool.fp8 ? "_fp8" : "");
        return SFA_ERR_UNSUPPORTED;
    }
    if (dt == SFA_DTYPE_F32) return launch_rest<float>(a, rg, SlotPool{}, nullptr, false, c.stream);
    if (dt == SFA_DTYPE_F16) return launch_rest<f16_t>(a, rg, c.pool, grp, *mfma, c.stream);
    return launch_rest<bf16_t>(a, rg, c.pool, grp, *mfma, c.stream);
}

}  // namespace

int decode_multi_check_head_dim(int64_t D, int dtype) {
    const int64_t row_bytes = D * dtype_size(dtype);
    if (D <= 0 || row_bytes % 16 != 0 || row_bytes > 1024) {
        set_error("decode_multi: head dim %lld (%lld bytes/row) must be a multiple of 16 bytes and <= 1024 bytes",
                  (long long)D, (long long)row_bytes);
        return SFA_ERR_UNSUPPORTED;
    }
    return SFA_OK;
}

size_t decode_multi_workspace(int64_t B, int64_t Hq, int64_t Hkv, int64_t n_new, int64_t Nkv, int64_t D, int dtype) {
    if (decode_multi_check_head_dim(D, dtype) != SFA_OK) return 0;
    if (B <= 0 || Hkv <= 0 || Hq % Hkv != 0 || n_new <= 0 || Nkv < n_new) return 0;
    const int64_t R = Hq / Hkv * n_new;
    const int64_t S = max_splits(B, Hkv, cdiv64(R, 32), Nkv);
    const size_t rows = (size_t)(B * Hkv * R);
    return 2 * al256(rows * S * sizeof(float)) + al256(rows * S * (size_t)D * sizeof(float));
}

int decode_multi_launch(const RingCall& c) {
    MultiArgs a = multi_args(c, true);
    a.want = (int)want_splits(a.B, a.Hkv, a.nrb);
    const MultiPlan p = multi_plan(a.sink_len, a.wl, a.n, a.want);
    a.T0 = p.T0, a.T1 = p.T1, a.T = p.T, a.tps = p.tps, a.S = p.S;
    // device state: (sink_len, window_len) = the full cache here; the grid covers the largest plan of any fill level and
    // every workgroup replans from its state row (workgroups of splits >= its S exit)
    a.Sw = c.state ? (int)max_splits(a.B, a.Hkv, a.nrb, c.sink_len + c.window_len + a.n) : a.S;
    const size_t rows = (size_t)a.B * a.Hkv * a.R;
    a.Mp = reinterpret_cast<float*>(c.workspace);
    a.Lp = reinterpret_cast<float*>((char*)c.workspace + al256(rows * a.Sw * sizeof(float)));
    a.Op = reinterpret_cast<float*>((char*)c.workspace + 2 * al256(rows * a.Sw * sizeof(float)));
    if ((int64_t)a.B * a.Hkv * a.Sw * a.nrb >= (1ll << 31) || cdiv64((int64_t)rows, 4) >= (1ll << 31) - 65536) {
        set_error("decode_multi: grid too large");
        return SFA_ERR_UNSUPPORTED;
    }
    bool mfma;
    const char* dname;
    const int st = launch_dtype(c, a, nullptr, &mfma, &dname);
    if (st) return st;
    const char* fam = c.parent ? "tree" : "multi";
    const char* cm = c.commit ? "_commit" : "";
    if (c.state) {
        const char* dyn = c.slots ? "_slots" : c.mode == RingState::Rows ? "_rows" : "_dyn";
        if (mfma) set_path("decode_%s_mfma_%s_d%d_rb%d%s%s", fam, dname, a.D, a.nrb, dyn, cm);
        else set_path("decode_%s_f32_%s_d%d%s%s", fam, dname, a.D, dyn, cm);
    } else {
        if (mfma) set_path("decode_%s_mfma_%s_d%d_rb%d_s%d%s", fam, dname, a.D, a.nrb, a.S, cm);
        else set_path("decode_%s_f32_%s_d%d_s%d%s", fam, dname, a.D, a.S, cm);
    }
    return SFA_OK;
}

namespace {

// host-known geometry of a packed call: nothing here depends on cu_q, the slots or the state
struct RaggedGeom {
    int64_t G, nrb, rows, Sw, P;     // P: bound of rows * Sw that sizes the partials
};

RaggedGeom ragged_geom(int64_t n_seq, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache) {
    RaggedGeom g;
    g.G = Hq / Hkv;
    g.nrb = cdiv64(g.G * T, 32) + n_seq;             // sum of ceil(G n_i / 32) over n_seq sequences of T rows in all
    g.rows = Hkv * T * g.G;
    g.Sw = max_splits(1, Hkv, g.nrb, Nkv_cache + T);   // bound of multi_plan's S over every fill and every n_i <= T
    // rows * Sw <= rows * (splits of the key count alone) and <= rows * ceil(2048 / (Hkv nrb)) <= rows + 2048 * 32
    // (G T / nrb <= 32): the smaller of two bounds that grow with T and Nkv_cache, so that the workspace size does too
    // (rows * Sw itself does not: Sw shrinks when the row blocks alone fill the device)
    const int64_t by_keys = cdiv64(cdiv64(Nkv_cache + T, kTile) + 2, kMinTiles);
    const int64_t p1 = g.rows * (by_keys < 1 ? 1 : by_keys), p2 = g.rows + kTargetWgs * 32;
    g.P = p1 < p2 ? p1 : p2;
    return g;
}

}  // namespace

size_t decode_ragged_workspace(int64_t n_seq, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache, int64_t D, int dtype) {
    if (decode_multi_check_head_dim(D, dtype) != SFA_OK) return 0;
    if (n_seq <= 0 || Hkv <= 0 || Hq <= 0 || Hq % Hkv != 0 || T <= 0 || Nkv_cache <= 0) return 0;
    if (n_seq >= (1ll << 30) || Hq * T >= (1ll << 30) || Nkv_cache >= (1ll << 30)) return 0;
    const RaggedGeom g = ragged_geom(n_seq, Hq, Hkv, T, Nkv_cache);
    return 2 * al256((size_t)g.P * sizeof(float)) + al256((size_t)g.P * (size_t)D * sizeof(float)) +
           al256((size_t)g.nrb * sizeof(int2)) + al256((size_t)T * sizeof(int));
}

namespace {

// host-known geometry of the groups of a packed call: nothing here depends on cu_g, cu_q, the slots or the state
struct GroupGeom {
    int64_t ngrb, want, Sgw, nsh, P;     // P = rows * Sgw sizes the group partials
};

GroupGeom group_geom(int64_t n_grp, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache) {
    GroupGeom g;
    const int64_t G = Hq / Hkv;
    g.ngrb = cdiv64(G * T, 32) + n_grp;              // sum of ceil(G n_g / 32) over n_grp groups of T rows in all
    g.want = want_splits(1, Hkv, g.ngrb);
    g.Sgw = max_splits(1, Hkv, g.ngrb, Nkv_cache);   // bound of multi_plan(0, Lg, 0, want).S over Lg <= Wc <= Nkv_cache
    g.nsh = (Hkv * g.Sgw * g.ngrb + 7) / 8 * 8;
    g.P = Hkv * T * G * g.Sgw;
    return g;
}

}  // namespace

// the workspace of a grouped call: that of the ungrouped call, then the group partials and the four tables of
// group_prep_kernel (gblk, glg, gseq and its own mrow)
size_t decode_ragged_group_workspace(int64_t n_seq, int64_t n_grp, int64_t Hq, int64_t Hkv, int64_t T, int64_t Nkv_cache,
                                     int64_t D, int dtype) {
    const size_t base = decode_ragged_workspace(n_seq, Hq, Hkv, T, Nkv_cache, D, dtype);
    if (base == 0 || n_grp <= 0 || n_grp >= (1ll << 30) || dtype == SFA_DTYPE_F32 || !mfma_head_dim((int)D)) return 0;
    const GroupGeom g = group_geom(n_grp, Hq, Hkv, T, Nkv_cache);
    return base + 2 * al256((size_t)g.P * sizeof(float)) + al256((size_t)g.P * (size_t)D * sizeof(float)) +
           al256((size_t)g.ngrb * sizeof(int2)) + al256((size_t)n_grp * sizeof(int2)) + 2 * al256((size_t)n_seq * sizeof(int));
}

int decode_ragged_launch(const RingCall& c) {
    const int64_t T = c.q->shape[2];
    const RaggedGeom g = ragged_geom(c.n_seq, c.q->shape[1], c.k_new->shape[1], T, c.sink_len + c.window_len);
    // B = 1; n / R: the pack's bounds here, every workgroup (wave) replaces them with its sequence's n_i and G * n_i
    MultiArgs a = multi_args(c, true);
    a.nrb = (int)g.nrb;
    a.want = (int)want_splits(1, a.Hkv, g.nrb);     // one value for the call: a sequence's plan depends on the call's
    a.Sw = (int)g.Sw;                               // shape and on its own (state row, n_i), not on its neighbours
    char* ws = (char*)c.workspace;
    a.Mp = reinterpret_cast<float*>(ws);
    a.Lp = reinterpret_cast<float*>(ws + al256((size_t)g.P * sizeof(float)));
    a.Op = reinterpret_cast<float*>(ws + 2 * al256((size_t)g.P * sizeof(float)));
    char* tab = ws + 2 * al256((size_t)g.P * sizeof(float)) + al256((size_t)g.P * (size_t)a.D * sizeof(float));
    int2* blk = reinterpret_cast<int2*>(tab);
    int* rowseq = reinterpret_cast<int*>(tab + al256((size_t)g.nrb * sizeof(int2)));
    const int admit = (c.flags & SFA_FLAG_RAGGED_ADMIT) ? 1 : 0;
    const RaggedArgs rg{c.cu_q, blk, rowseq, c.n_seq, (int)T, admit, c.commit_seq};
    a.pstride = 0;                                  // parent is packed like q: a tree sequence reads parent + its first row
    if ((int64_t)a.Hkv * a.Sw * g.nrb >= (1ll << 31) || cdiv64(g.rows, 4) >= (1ll << 31) - 65536 ||
        cdiv64(g.rows, 4) + cdiv64((int64_t)a.Hkv * T * (a.D * 4 / 16), 256) >= (1ll << 31)) {
        set_error("decode_ragged: grid too large");
        return SFA_ERR_UNSUPPORTED;
    }
    ragged_prep_kernel<<<1, 1024, 0, c.stream>>>(rg, blk, rowseq, a.G, a.nrb);
    int st;
    if ((st = launch_status("ragged_prep"))) return st;
    GroupArgs gr{};
    if (c.cu_g) {       // fork groups: the second partial area and the tables lie behind the ungrouped call's workspace
        const GroupGeom gg = group_geom(c.n_grp, c.q->shape[1], a.Hkv, T, c.sink_len + c.window_len);
        char* gw = ws + decode_ragged_workspace(c.n_seq, c.q->shape[1], a.Hkv, T, c.sink_len + c.window_len, a.D, c.q->dtype);
        gr.cu_g = c.cu_g, gr.n_grp = c.n_grp;
        gr.Mg = reinterpret_cast<float*>(gw);
        gr.Lg = reinterpret_cast<float*>(gw + al256((size_t)gg.P * sizeof(float)));
        gr.Og = reinterpret_cast<float*>(gw + 2 * al256((size_t)gg.P * sizeof(float)));
        char* gt = gw + 2 * al256((size_t)gg.P * sizeof(float)) + al256((size_t)gg.P * (size_t)a.D * sizeof(float));
        int2* gblk = reinterpret_cast<int2*>(gt);
        int2* glg = reinterpret_cast<int2*>(gt + al256((size_t)gg.ngrb * sizeof(int2)));
        int* gseq = reinterpret_cast<int*>(gt + al256((size_t)gg.ngrb * sizeof(int2)) + al256((size_t)c.n_grp * sizeof(int2)));
        int* mrow = gseq + al256((size_t)c.n_seq * sizeof(int)) / sizeof(int);     // group_prep_kernel's own
        gr.gblk = gblk, gr.glg = glg, gr.gseq = gseq;
        gr.ngrb = (int)gg.ngrb, gr.Sgw = (int)gg.Sgw, gr.want_g = (int)gg.want, gr.nsh = (int)gg.nsh;
        if ((int64_t)a.Hkv * a.Sw * g.nrb + gg.nsh >= (1ll << 31)) {
            set_error("decode_ragged: grid too large");
            return SFA_ERR_UNSUPPORTED;
        }
        // reads the state rows and the table; the advance stays the trailing launch (the state-ordering rule)
        group_prep_kernel<<<c.n_grp, 1024, 0, c.stream>>>(rg, gr, page_args(c.pool.pt), gblk, glg, gseq, mrow, c.state,
                                                          c.slots, a.npool, a.wc, a.G);
        if ((st = launch_status("group_prep"))) return st;
    }
    bool mfma;
    const char* dname;
    if ((st = launch_dtype(c, a, &rg, &mfma, &dname, c.cu_g ? &gr : nullptr))) return st;
    const char *ad = admit ? "_admit" : "", *cm = c.commit ? "_commit" : "";
    const char* fam = c.parent ? "tree" : "multi";
    if (mfma) set_path("decode_%s_mfma_%s_d%d_rb%d_ragged%s%s%s%s", fam, dname, a.D, a.nrb, ad, cm, c.cu_g ? "_group" : "", pool_tag(c.pool));
    else set_path("decode_%s_f32_%s_d%d_ragged%s%s", fam, dname, a.D, ad, cm);
    return SFA_OK;
}

int ring_commit_dyn_launch(const RingCall& c) {
    const MultiArgs a = multi_args(c, false);
    const bool rows = c.mode == RingState::Rows;
    const int es = dtype_size(c.k_new->dtype);
    if (c.cu_q) {       // the pack: one piece per (KV head, packed row, 16 bytes), the advance by clamp(count[i], 0, n_i)
        const RaggedArgs rg{c.cu_q, nullptr, nullptr, c.n_seq, a.n, 0, nullptr};
        const int64_t nb = cdiv64((int64_t)a.Hkv * a.n * (a.D * (int64_t)es / 16), 256);
        if (nb >= (1ll << 31)) {
            set_error("ring_commit: grid too large");
            return SFA_ERR_UNSUPPORTED;
        }
        int st;
        if (nb > 0) {
            const dim3 grid((unsigned)nb);
            dispatch_pool(c.pool, [&](auto p, auto... tail) {
                using P = decltype(p);
                ring_commit_ragged_kernel<typename P::Q, P::Paged><<<grid, 256, 0, c.stream>>>(a, rg, c.count, es, tail...);
            }, c.k_new->dtype);
            if ((st = launch_status("ring_commit_path_ragged"))) return st;
        }
        if ((st = launch_advance(a, c.count, &rg, c.stream))) return st;   // after every reader of the state
        set_path("ring_commit_path_ragged_slots%s", pool_tag(c.pool));
        return SFA_OK;
    }
    const int64_t ncm = a.n < a.wc ? a.n : a.wc;
    const int64_t nblk = cdiv64((int64_t)a.B * a.Hkv * ncm * (a.D * (int64_t)es / 16), 256);
    if (nblk >= (1ll << 31)) {
        set_error("ring_commit: grid too large");
        return SFA_ERR_UNSUPPORTED;
    }
    int st;
    if (nblk > 0) {
        const dim3 grid((unsigned)nblk);
        if (c.slots && c.path) ring_commit_slots_kernel<true><<<grid, 256, 0, c.stream>>>(a, c.count, es);
        else if (c.slots) ring_commit_slots_kernel<false><<<grid, 256, 0, c.stream>>>(a, c.count, es);
        else if (c.path) ring_commit_path_kernel<<<grid, 256, 0, c.stream>>>(a, c.count, es);
        else ring_commit_kernel<<<grid, 256, 0, c.stream>>>(a, c.count, es);
        if ((st = launch_status(c.path ? "ring_commit_path" : "ring_commit"))) return st;
    }
    // after every reader of the state
    if ((st = launch_advance(a, c.count, nullptr, c.stream))) return st;
    if (c.path) set_path(c.slots ? "ring_commit_path_slots" : rows ? "ring_commit_path_rows" : "ring_commit_path_dyn");
    else set_path(c.slots ? "ring_commit_slots" : rows ? "ring_commit_rows" : "ring_commit_dyn");
    return SFA_OK;
}

int ring_fill_varlen_launch(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                            const sfa_tensor* window_v, const sfa_tensor* k, const sfa_tensor* v, const int32_t* cu,
                            int n_seq, int32_t* state, hipStream_t stream, const int32_t* slots, const SlotPool& pool) {
    const int es = dtype_size(k->dtype);
    const int Hkv = (int)k->shape[1], ns = (int)sink_k->shape[2], wc = (int)window_k->shape[2];
    const int cpr = (int)(k->shape[3] * es / 16);
    const int64_t nblk = cdiv64((int64_t)n_seq * Hkv * (ns + wc) * cpr, 256);
    if (nblk >= (1ll << 31)) {
        set_error("ring_fill_varlen: grid too large");
        return SFA_ERR_UNSUPPORTED;
    }
    if (nblk > 0) {
        auto launch = [&](auto kernel, auto... tail) {
            kernel<<<dim3((unsigned)nblk), 256, 0, stream>>>(
                make_view(sink_k), make_view(sink_v), make_view(window_k), make_view(window_v), make_view(k), make_view(v),
                cu, state, n_seq, Hkv, ns, wc, (int)k->shape[2], cpr, es, slots, slots ? (int)sink_k->shape[0] : 0, tail...);
        };
        if (!slots) launch(ring_fill_varlen_kernel<false>);     // the API: a pool is all zero without slots
        else
            dispatch_pool(pool, [&](auto p, auto... tail) {
                using P = decltype(p);
                launch(ring_fill_varlen_kernel<true, typename P::Q, P::Paged, decltype(tail)...>, tail...);
            }, k->dtype);
        int st;
        if ((st = launch_status("ring_fill_varlen"))) return st;
    }
    set_path("ring_fill_varlen%s%s", slots ? "_slots" : "", pool_tag(pool));
    return SFA_OK;
}

int ring_copy_slots_launch(const sfa_tensor* const src[4], const int32_t* src_state, const sfa_tensor* const dst[4],
                           int32_t* dst_state, const int32_t* src_slots, const int32_t* dst_slots, int n_pairs,
                           hipStream_t stream, const SlotPool& src_pool, const SlotPool& dst_pool) {
    const sfa_tensor *sk = src[0], *wk = src[2];
    const int es = dtype_size(wk->dtype);
    const int Hkv = (int)wk->shape[1], ns = (int)sk->shape[2], wc = (int)wk->shape[2];
    const int cpr = (int)(wk->shape[3] * es / 16);
    const int64_t nblk = cdiv64((int64_t)(ns + wc) * cpr, 256 * kCopyPieces);
    const int64_t grid = (int64_t)n_pairs * Hkv * nblk;
    if (grid >= (1ll << 31)) {
        set_error("ring_copy_slots: grid too large");
        return SFA_ERR_UNSUPPORTED;
    }
    if (grid > 0) {
        const CopyPools s{make_view(src[0]), make_view(src[1]), make_view(src[2]), make_view(src[3]),
                          const_cast<int*>(src_state), src_slots, (int)wk->shape[0]};
        const CopyPools d{make_view(dst[0]), make_view(dst[1]), make_view(dst[2]), make_view(dst[3]),
                          dst_state, dst_slots, (int)dst[2]->shape[0]};
        if (src_pool.pt.table)
            ring_copy_slots_kernel<true><<<dim3((unsigned)grid), 256, 0, stream>>>(
                s, d, Hkv, ns, wc, cpr, es, (int)nblk, src_state == dst_state ? 1 : 0, page_args(src_pool.pt), page_args(dst_pool.pt));
        else
            ring_copy_slots_kernel<<<dim3((unsigned)grid), 256, 0, stream>>>(s, d, Hkv, ns, wc, cpr, es, (int)nblk,
                                                                             src_state == dst_state ? 1 : 0);
        int st;
        if ((st = launch_status("ring_copy_slots"))) return st;
    }
    set_path("ring_copy_slots%s", pool_tag(src_pool));
    return SFA_OK;
}

int ring_export_slots_launch(const sfa_tensor* sink_k, const sfa_tensor* sink_v, const sfa_tensor* window_k,
                             const sfa_tensor* window_v, const sfa_tensor* k_out, const sfa_tensor* v_out, const int32_t* cu,
                             int n_seq, const int32_t* state, const int32_t* slots, int32_t* pos_out, hipStream_t stream,
                             const SlotPool& pool) {
    const int es = dtype_size(k_out->dtype);
    const int Hkv = (int)k_out->shape[1], T = (int)k_out->shape[2];
    const int cpr = (int)(k_out->shape[3] * es / 16);
    const int64_t nblk = cdiv64((int64_t)T * cpr, 256 * kExportPieces);      // the pack's pieces per head: < 2^30 (host check)
    const int64_t grid = (int64_t)Hkv * nblk;
    if (grid >= (1ll << 31)) {
        set_error("ring_export_slots: grid too large");
        return SFA_ERR_UNSUPPORTED;
    }
    if (grid > 0) {
        const ExportArgs a{make_view(sink_k), make_view(sink_v), make_view(window_k), make_view(window_v), make_view(k_out),
                           make_view(v_out), cu, state, slots, pos_out, n_seq, (int)sink_k->shape[0], Hkv,
                           (int)sink_k->shape[2], (int)window_k->shape[2], T, cpr, es, (int)nblk};
        dispatch_pool(pool, [&](auto p, auto... tail) {
            using P = decltype(p);
            ring_export_slots_kernel<typename P::Q, P::Paged><<<dim3((unsigned)grid), 256, 0, stream>>>(a, tail...);
        }, k_out->dtype);
        int st;
        if ((st = launch_status("ring_export_slots"))) return st;
    }
    set_path("ring_export_slots%s", pool_tag(pool));
    return SFA_OK;
}

int ring_share_slots_launch(const sfa_tensor* src_sink_k, const sfa_tensor* src_sink_v, const int32_t* src_state,
                            const sfa_tensor* dst_sink_k, const sfa_tensor* dst_sink_v, int32_t* dst_state,
                            const int32_t* src_slots, const int32_t* dst_slots, int n_pairs, hipStream_t stream) {
    const int es = dtype_size(src_sink_k->dtype);
    const int Hkv = (int)src_sink_k->shape[1], ns = (int)src_sink_k->shape[2];
    const int cpr = (int)(src_sink_k->shape[3] * es / 16);
    const int64_t nblk = ns > 0 ? cdiv64((int64_t)ns * cpr, 256) : 1;      // num_sink == 0: the state row alone
    const int64_t grid = (int64_t)n_pairs * Hkv * nblk;
    if (grid >= (1ll << 31)) {
        set_error("ring_share_slots: grid too large");
        return SFA_ERR_UNSUPPORTED;
    }
    if (grid > 0) {
        const CopyPools s{make_view(src_sink_k), make_view(src_sink_v), View{}, View{}, const_cast<int*>(src_state),
                          src_slots, (int)src_sink_k->shape[0]};
        const CopyPools d{make_view(dst_sink_k), make_view(dst_sink_v), View{}, View{}, dst_state, dst_slots,
                          (int)dst_sink_k->shape[0]};
        ring_share_slots_kernel<<<dim3((unsigned)grid), 256, 0, stream>>>(s, d, Hkv, ns, cpr, es, (int)nblk,
                                                                          src_state == dst_state ? 1 : 0);
        int st;
        if ((st = launch_status("ring_share_slots"))) return st;
    }
    set_path("ring_share_slots_paged");
    return SFA_OK;
}

int pages_copy_launch(const sfa_tensor* window_k, const sfa_tensor* window_v, const int32_t* src_pages,
                      const int32_t* dst_pages, int n_pairs, hipStream_t stream) {
    const int es = dtype_size(window_k->dtype);
    const int Hkv = (int)window_k->shape[1], P = (int)window_k->shape[2];
    const int cpr = (int)(window_k->shape[3] * es / 16);
    const int64_t per_page = (int64_t)Hkv * P * cpr;        // < 2^30: checked on the host
    const int64_t nblk = cdiv64(per_page, 256 * kPagePieces);
    const int64_t grid = (int64_t)n_pairs * nblk;
    if (grid >= (1ll << 31)) {
        set_error("pages_copy: grid too large");
        return SFA_ERR_UNSUPPORTED;
    }
    if (grid > 0) {
        pages_copy_kernel<<<dim3((unsigned)grid), 256, 0, stream>>>(make_view(window_k), make_view(window_v), src_pages,
                                                                    dst_pages, (int)window_k->shape[0], P, cpr, es,
                                                                    (int)nblk, (int)per_page);
        int st;
        if ((st = launch_status("pages_copy"))) return st;
    }
    set_path("pages_copy");
    return SFA_OK;
}

}  // namespace sfa
