"""ctypes binding of libsfa.so (C ABI in include/sfa.h).

The shared library holds the hand-written gfx950 HIP kernels.  There is NO
fallback: if the library is missing or a call fails, this module raises.
Build it with ``make -C sink-flash-attention-kernel_amd`` (or
``python -c "import __graft_entry__ as g; g.build()"`` from the repo root).
"""
from __future__ import annotations

import ctypes
import os
import struct
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFA_LIB_PATH") or os.path.join(_HERE, "libsfa.so")   # env: A/B builds in development

SFA_DTYPE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
SFA_DTYPE_FP8_E4M3 = 3        # OCP e4m3fn: the cache buffers of an FP8 pool only (the *_fp8_slots calls, sfa_ring_copy_slots)
_DESC_DTYPE = {**SFA_DTYPE, torch.float8_e4m3fn: SFA_DTYPE_FP8_E4M3}
FLAG_FORCE_GENERIC = 0x1
FLAG_DECODE_ONE_PASS = 0x4
FLAG_BWD_OVERLAP = 0x8        # dQ kernel of a small grid on the library's side stream (include/sfa.h)
FLAG_BWD_DKDV_ASM = 0x10      # dispatch override: hand-placed dK/dV kernel
FLAG_BWD_DKDV_WS = 0x20       # dispatch override: wave-specialised compiled dK/dV kernel
FLAG_RAGGED_ADMIT = 0x40      # sfa_decode_ring_ragged_slots: a sequence on a fresh slot (seen == 0) is admitted in the call
ABI_VERSION = 2

# flags every backward of the ops passes to sfa_bwd / sfa_bwd_varlen (and to the workspace query): the overlap is ON by
# default here - the C entry points do nothing of the kind unless asked
_bwd_flags = FLAG_BWD_OVERLAP


def set_backward_options(overlap=None, dkdv=None):
    """Process-wide options of the ops' backward pass.  overlap: True / False - dQ kernel of small grids on the library's
    side stream (default True).  dkdv: None (the library's rule) / "asm" (hand-placed kernel) / "ws" (wave-specialised
    compiled kernel): the dispatch override the parity tests use.  Returns the previous (overlap, dkdv)."""
    global _bwd_flags
    prev = (bool(_bwd_flags & FLAG_BWD_OVERLAP),
            "asm" if _bwd_flags & FLAG_BWD_DKDV_ASM else ("ws" if _bwd_flags & FLAG_BWD_DKDV_WS else None))
    f = _bwd_flags
    if overlap is not None:
        f = (f | FLAG_BWD_OVERLAP) if overlap else (f & ~FLAG_BWD_OVERLAP)
    if dkdv is not None or overlap is None:
        f &= ~(FLAG_BWD_DKDV_ASM | FLAG_BWD_DKDV_WS)
        if dkdv == "asm":
            f |= FLAG_BWD_DKDV_ASM
        elif dkdv == "ws":
            f |= FLAG_BWD_DKDV_WS
        elif dkdv not in (None, "rule"):
            raise ValueError("dkdv must be None, 'rule', 'asm' or 'ws'")
    _bwd_flags = f
    return prev


def bwd_flags(flags=0) -> int:
    return flags | _bwd_flags


class SfaTensor(ctypes.Structure):
    _fields_ = [
        ("ptr", ctypes.c_void_p),
        ("shape", ctypes.c_int64 * 4),
        ("stride", ctypes.c_int64 * 4),
        ("dtype", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


_lib = None
_lock = threading.Lock()


def _bind(lib):
    P = ctypes.POINTER(SfaTensor)
    vp, i32, u32, f32, sz, i64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_size_t,
                                   ctypes.c_int64)
    lib.sfa_abi_version.restype = i32
    lib.sfa_abi_version.argtypes = []
    lib.sfa_last_error.restype = ctypes.c_char_p
    lib.sfa_last_error.argtypes = []
    lib.sfa_last_path.restype = ctypes.c_char_p
    lib.sfa_last_path.argtypes = []
    lib.sfa_debug_set_ptr.restype = i32
    lib.sfa_debug_set_ptr.argtypes = [ctypes.c_void_p]
    lib.sfa_debug_set_variant.restype = i32
    lib.sfa_debug_set_variant.argtypes = [i32, i32]
    lib.sfa_debug_set_stage_events.restype = i32
    lib.sfa_debug_set_stage_events.argtypes = [ctypes.POINTER(ctypes.c_void_p), i32]
    lib.sfa_fwd.restype = i32
    lib.sfa_fwd.argtypes = [P, P, P, P, vp, vp, i32, i32, f32, u32, vp]
    lib.sfa_bwd_workspace_bytes.restype = sz
    lib.sfa_bwd_workspace_bytes.argtypes = [i64, i64, i64, i64, i64, i32, i32, i32, u32]
    lib.sfa_bwd.restype = i32
    lib.sfa_bwd.argtypes = [P, P, P, P, P, vp, vp, P, P, P, vp, vp, sz, i32, i32, f32, u32, vp]
    lib.sfa_varlen_supported.restype = i32
    lib.sfa_varlen_supported.argtypes = [i32, i64]
    lib.sfa_fwd_varlen.restype = i32
    lib.sfa_fwd_varlen.argtypes = [P, P, P, P, vp, vp, vp, i32, i32, i32, i32, f32, u32, vp]
    lib.sfa_bwd_varlen.restype = i32
    lib.sfa_bwd_varlen.argtypes = [P, P, P, P, P, vp, vp, P, P, P, vp, vp, i32, i32, vp, sz, i32, i32, f32, u32, vp]
    lib.sfa_decode_workspace_bytes.restype = sz
    lib.sfa_decode_workspace_bytes.argtypes = [i64, i64, i64, i64, i64, i32]
    lib.sfa_decode.restype = i32
    lib.sfa_decode.argtypes = [P, P, P, P, vp, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring.restype = i32
    lib.sfa_decode_ring.argtypes = [P, P, P, i64, P, P, i64, P, vp, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_step.restype = i32
    lib.sfa_decode_ring_step.argtypes = [P, P, P, i64, P, P, i64, i64, P, P, P, vp, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_step_dyn.restype = i32
    lib.sfa_decode_ring_step_dyn.argtypes = [P, P, P, P, P, P, P, P, vp, vp, vp, sz, f32, u32, vp]
    lib.sfa_decode_multi_workspace_bytes.restype = sz
    lib.sfa_decode_multi_workspace_bytes.argtypes = [i64, i64, i64, i64, i64, i64, i32]
    lib.sfa_decode_ring_multi.restype = i32
    lib.sfa_decode_ring_multi.argtypes = [P, P, P, i64, P, P, i64, i64, P, P, P, vp, i32, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_multi_dyn.restype = i32
    lib.sfa_decode_ring_multi_dyn.argtypes = [P, P, P, P, P, P, P, P, vp, i32, vp, vp, sz, f32, u32, vp]
    lib.sfa_ring_commit_dyn.restype = i32
    lib.sfa_ring_commit_dyn.argtypes = [P, P, P, P, vp, vp, vp]
    lib.sfa_decode_ring_step_rows.restype = i32
    lib.sfa_decode_ring_step_rows.argtypes = [P, P, P, P, P, P, P, P, vp, vp, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_multi_rows.restype = i32
    lib.sfa_decode_ring_multi_rows.argtypes = [P, P, P, P, P, P, P, P, vp, i32, vp, vp, sz, f32, u32, vp]
    lib.sfa_ring_commit_rows.restype = i32
    lib.sfa_ring_commit_rows.argtypes = [P, P, P, P, vp, vp, vp]
    lib.sfa_decode_ring_tree.restype = i32
    lib.sfa_decode_ring_tree.argtypes = [P, P, P, i64, P, P, i64, i64, P, P, P, vp, vp, i64, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_tree_dyn.restype = i32
    lib.sfa_decode_ring_tree_dyn.argtypes = [P, P, P, P, P, P, P, P, vp, vp, i64, vp, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_tree_rows.restype = i32
    lib.sfa_decode_ring_tree_rows.argtypes = [P, P, P, P, P, P, P, P, vp, vp, i64, vp, vp, sz, f32, u32, vp]
    lib.sfa_ring_commit_path_dyn.restype = i32
    lib.sfa_ring_commit_path_dyn.argtypes = [P, P, P, P, vp, vp, i64, vp, vp]
    lib.sfa_ring_commit_path_rows.restype = i32
    lib.sfa_ring_commit_path_rows.argtypes = [P, P, P, P, vp, vp, i64, vp, vp]
    lib.sfa_ring_fill_varlen.restype = i32
    lib.sfa_ring_fill_varlen.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp]
    # slot-indexed siblings (continuous batching): the rows call plus `slots` after `state`
    lib.sfa_decode_ring_step_slots.restype = i32
    lib.sfa_decode_ring_step_slots.argtypes = [P, P, P, P, P, P, P, P, vp, vp, vp, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_multi_slots.restype = i32
    lib.sfa_decode_ring_multi_slots.argtypes = [P, P, P, P, P, P, P, P, vp, i32, vp, vp, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_tree_slots.restype = i32
    lib.sfa_decode_ring_tree_slots.argtypes = [P, P, P, P, P, P, P, P, vp, vp, i64, vp, vp, vp, sz, f32, u32, vp]
    lib.sfa_ring_commit_slots.restype = i32
    lib.sfa_ring_commit_slots.argtypes = [P, P, P, P, vp, vp, vp, vp]
    lib.sfa_ring_commit_path_slots.restype = i32
    lib.sfa_ring_commit_path_slots.argtypes = [P, P, P, P, vp, vp, i64, vp, vp, vp]
    lib.sfa_ring_fill_varlen_slots.restype = i32
    lib.sfa_ring_fill_varlen_slots.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp, vp]
    # packed ragged step over a pool: the slots call plus `cu_q`, `n_seq` after `slots`
    lib.sfa_decode_ragged_workspace_bytes.restype = sz
    lib.sfa_decode_ragged_workspace_bytes.argtypes = [i64, i64, i64, i64, i64, i64, i32]
    lib.sfa_decode_ring_ragged_slots.restype = i32
    lib.sfa_decode_ring_ragged_slots.argtypes = [P, P, P, P, P, P, P, P, vp, i32, vp, vp, vp, i32, vp, sz, f32, u32, vp]
    # ... with draft trees (`parent`) and per-sequence commit (`commit_seq`) before `commit`; the packed path commit
    lib.sfa_decode_ring_ragged_tree_slots.restype = i32
    lib.sfa_decode_ring_ragged_tree_slots.argtypes = [P, P, P, P, P, P, P, P, vp, vp, vp, i32, vp, vp, vp, i32, vp, sz, f32,
                                                      u32, vp]
    lib.sfa_ring_commit_path_ragged_slots.restype = i32
    lib.sfa_ring_commit_path_ragged_slots.argtypes = [P, P, P, P, vp, vp, vp, i32, vp, vp, vp]
    # FP8 pool: the packed step, the packed commit and the slot fill plus `kv_scale` (device f32 [2, H_kv]) before the tail
    lib.sfa_decode_ring_ragged_fp8_slots.restype = i32
    lib.sfa_decode_ring_ragged_fp8_slots.argtypes = [P, P, P, P, P, P, P, P, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, sz,
                                                     f32, u32, vp]
    lib.sfa_ring_commit_path_ragged_fp8_slots.restype = i32
    lib.sfa_ring_commit_path_ragged_fp8_slots.argtypes = [P, P, P, P, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.sfa_ring_fill_varlen_fp8_slots.restype = i32
    lib.sfa_ring_fill_varlen_fp8_slots.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp, vp, vp]
    # slot copy (fork / park): source pool + state, destination pool + state, src_slots, dst_slots, n_pairs, stream
    lib.sfa_ring_copy_slots.restype = i32
    lib.sfa_ring_copy_slots.argtypes = [P, P, P, P, vp, P, P, P, P, vp, vp, vp, i32, vp]
    # paged pool: the packed step, the packed commit (plus n_slots), the slot fill and the slot copy (a pair per side) plus
    # (`page_table` device int32 [S, table_stride], `table_stride`) before the tail
    lib.sfa_decode_ring_ragged_paged_slots.restype = i32
    lib.sfa_decode_ring_ragged_paged_slots.argtypes = [P, P, P, P, P, P, P, P, vp, vp, vp, i32, vp, vp, vp, i32, vp, i32, vp,
                                                       sz, f32, u32, vp]
    lib.sfa_ring_commit_path_ragged_paged_slots.restype = i32
    lib.sfa_ring_commit_path_ragged_paged_slots.argtypes = [P, P, P, P, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp]
    lib.sfa_ring_fill_varlen_paged_slots.restype = i32
    lib.sfa_ring_fill_varlen_paged_slots.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp, vp, i32, vp]
    lib.sfa_ring_copy_paged_slots.restype = i32
    lib.sfa_ring_copy_paged_slots.argtypes = [P, P, P, P, vp, P, P, P, P, vp, vp, vp, i32, vp, i32, vp, i32, vp]
    # shared fork of a paged pool: the unpaged half of the slot copy (sinks + state of each side, no ring, no table), and
    # the copy of whole pages (page buffers, src_pages, dst_pages, n_pairs, stream) in front of a store into a shared page
    lib.sfa_ring_share_paged_slots.restype = i32
    lib.sfa_ring_share_paged_slots.argtypes = [P, P, vp, P, P, vp, vp, vp, i32, vp]
    lib.sfa_pages_copy.restype = i32
    lib.sfa_pages_copy.argtypes = [P, P, vp, vp, i32, vp]
    # paged FP8 pool: the paged step, commit and fill plus `kv_scale` behind the table arguments (the copy is the paged one)
    lib.sfa_decode_ring_ragged_paged_fp8_slots.restype = i32
    lib.sfa_decode_ring_ragged_paged_fp8_slots.argtypes = [P, P, P, P, P, P, P, P, vp, vp, vp, i32, vp, vp, vp, i32, vp, i32,
                                                           vp, vp, sz, f32, u32, vp]
    lib.sfa_ring_commit_path_ragged_paged_fp8_slots.restype = i32
    lib.sfa_ring_commit_path_ragged_paged_fp8_slots.argtypes = [P, P, P, P, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp]
    lib.sfa_ring_fill_varlen_paged_fp8_slots.restype = i32
    lib.sfa_ring_fill_varlen_paged_fp8_slots.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp, vp, i32, vp, vp]
    # fork groups on a paged pool: the paged step without `parent`, plus (`cu_g` device int32 [n_grp + 1], `n_grp`) behind
    # (`cu_q`, `n_seq`); the workspace query takes n_grp behind n_seq
    lib.sfa_decode_ragged_group_workspace_bytes.restype = sz
    lib.sfa_decode_ragged_group_workspace_bytes.argtypes = [i64, i64, i64, i64, i64, i64, i64, i32]
    lib.sfa_decode_ring_ragged_group_paged_slots.restype = i32
    lib.sfa_decode_ring_ragged_group_paged_slots.argtypes = [P, P, P, P, P, P, P, P, vp, vp, i32, vp, vp, vp, i32, vp, i32,
                                                             vp, i32, vp, sz, f32, u32, vp]
    lib.sfa_decode_ring_ragged_group_paged_fp8_slots.restype = i32
    lib.sfa_decode_ring_ragged_group_paged_fp8_slots.argtypes = [P, P, P, P, P, P, P, P, vp, vp, i32, vp, vp, vp, i32, vp,
                                                                 i32, vp, i32, vp, vp, sz, f32, u32, vp]
    # export (the inverse of the slot fills): the pool buffers, k_out / v_out, cu, n_seq, state, slots, pos_out, then the
    # table arguments and / or kv_scale of the pool's kind as the fills take them, then stream
    lib.sfa_ring_export_slots.restype = i32
    lib.sfa_ring_export_slots.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp, vp, vp]
    lib.sfa_ring_export_fp8_slots.restype = i32
    lib.sfa_ring_export_fp8_slots.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp, vp, vp, vp]
    lib.sfa_ring_export_paged_slots.restype = i32
    lib.sfa_ring_export_paged_slots.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp, vp, vp, i32, vp]
    lib.sfa_ring_export_paged_fp8_slots.restype = i32
    lib.sfa_ring_export_paged_fp8_slots.argtypes = [P, P, P, P, P, P, vp, i32, vp, vp, vp, vp, i32, vp, vp]


def lib():
    """Load (once) and return the ctypes handle; raises if libsfa.so is absent."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"sink_attention: {LIB_PATH} not found. The HIP extension is required (there is no "
                        "Python/CPU fallback). Build it with `make -C sink-flash-attention-kernel_amd`.")
                handle = ctypes.CDLL(LIB_PATH)
                _bind(handle)
                v = handle.sfa_abi_version()
                if v != ABI_VERSION:
                    raise RuntimeError(f"libsfa.so ABI version {v}, expected {ABI_VERSION}: rebuild the extension")
                _lib = handle
    return _lib


def last_path() -> str:
    return lib().sfa_last_path().decode()


_DESC = struct.Struct("P4q4qii")        # SfaTensor's layout: one pack instead of ten ctypes field stores (1 us against 5 per
assert _DESC.size == ctypes.sizeof(SfaTensor)   # descriptor; a backward call builds ten of them)


def desc(t: torch.Tensor) -> SfaTensor:
    """Describe a 4-D [B,H,N,D] tensor (any B/H/N strides, unit D stride)."""
    return SfaTensor.from_buffer_copy(_DESC.pack(t.data_ptr(), *t.shape, *t.stride(), _DESC_DTYPE[t.dtype], 0))


def check(status: int, what: str):
    if status != 0:
        msg = lib().sfa_last_error().decode()
        kind = "argument/support error" if status < 0 else "HIP error"
        raise RuntimeError(f"{what} failed ({kind} {status}): {msg}")


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "sink_attention runs only on MI355X (HIP) tensors; got a CPU tensor and there is no CPU fallback")


def unit_inner(t: torch.Tensor) -> torch.Tensor:
    """Kernels take arbitrary B/H/N strides but need the head dim contiguous."""
    if t.stride(-1) != 1 and t.shape[-1] > 1:
        return t.contiguous()
    return t


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream
