"""ctypes binding of libbeast_hip.so (the C-ABI in include/beast_hip.h).

The library is the only compute path: if it is missing, or the tensors are not on
a ROCm GPU, calls raise ``RuntimeError`` -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import NamedTuple, Optional

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# BEAST_LIB: another build of the same library (tools/asan: the host-AddressSanitizer build)
LIB_PATH = os.environ.get("BEAST_LIB") or os.path.join(_PKG, "libbeast_hip.so")

BEAST_OK = 0
BEAST_E_INVALID = -1
BEAST_E_HIP = -2
BEAST_E_UNSUPPORTED = -3
BEAST_E_WORKSPACE = -4
ABI_VERSION = 6
OPT_GENERIC_KERNELS = 1
OPT_BLOCK_WAVES = 2
OPT_MERGE_LDS_MIN = 3
OPT_BPE_ENCODE_MODE = 5
OPT_BPE_DEDUP_KEY_BITS = 6
OPT_BPE_TRAIN_HOST_LOOP = 7
OPT_LAST_CODEC_LAUNCH = 8   # read-only
OPT_LAST_LAUNCH_GRID = 9    # read-only
# beast_bpe_loop_batch flags, and the int32 words of the loop state a host reads
BPE_BATCH_INIT = 1
BPE_BATCH_NO_MERGE = 2
BPE_BATCH_NO_APPLY = 4
BPE_STATE_ACTIVE = 0
BPE_STATE_VCUR = 1
BPE_STATE_NMERGES = 2
BPE_STATE_PASSES = 9
BPE_LOOP_P = 0x9E3779B97F4A7C15   # odd multiplier of the token-string hash (csrc/bpe_vocab.h LOOP_P)
# BEAST_LOGITS_*: the element types beast_logits_expect / _bwd and beast_xent_rows / _bwd read as they are
LOGITS_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

# kernel families of OPT_LAST_CODEC_LAUNCH (bits 0-3), in the header's order
CODEC_FAMILIES = (None, "encode_v", "encode_spec", "encode_dyn", "reconstruct_v", "reconstruct_spec",
                  "reconstruct_mfma", "reconstruct_rows")

_vp, _i64, _i32, _f32, _f64, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_size_t

# name -> (restype, argtypes); kept in the order of include/beast_hip.h
SIGNATURES = {
    "beast_abi_version": (_i32, []),
    "beast_last_error": (C.c_char_p, []),
    "beast_set_option": (_i32, [_i32, _i32]),
    "beast_get_option": (_i32, [_i32]),
    "beast_bspline_basis_f32": (_i32, [_vp, _i64, _f32, _f32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "beast_bspline_basis_deriv_f32": (_i32, [_vp, _i64, _f32, _f32, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "beast_bspline_projection_f64": (_i32, [_vp, _i32, _i32, _f64, _vp, _vp]),
    "beast_encode_f32": (_i32, [_vp, _i64, _i32, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp,
                                _i32, _i64, _vp, _vp, _vp]),
    "beast_encode_list_f32": (_i32, [_vp, _i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "beast_quantize_f32": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp]),
    "beast_encode_rows_f32": (_i32, [_vp, _i64, _i32, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _f32,
                                     _f32, _vp, _i32, _vp, _i32, _i32, _i32, _f64, _vp, _vp, _i32, _i64, _vp, _vp,
                                     _vp]),
    "beast_encode_windows_f32": (_i32, [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _i32,
                                        _vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp]),
    "beast_reconstruct_windows_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _i32, _vp,
                                             _vp, _i64, _vp, _f32, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "beast_blend_candidates_host": (_i32, [_vp, _vp, _i64, _i64, _i32, _i64, _i64, _vp, _vp]),
    "beast_blend_member_host": (_i32, [_i64, _i64, _i64, _i32, _i64]),
    "beast_cond_fixed_f32": (_i32, [_vp, _i64, _i32, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _i32, _i32, _f32, _i32,
                                    _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "beast_cond_add_f32": (_i32, [_vp, _i64, _i32, _i32, _vp, _i32, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "beast_reconstruct_f32": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32,
                                     _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "beast_reconstruct_derivs_f32": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _i64, _i32, _vp,
                                            _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "beast_reconstruct_derivs_bwd_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _i32,
                                                _vp, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "beast_logits_expect": (_i32, [_vp, _i32, _i64, _i32, _i32, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp]),
    "beast_logits_expect_bwd": (_i32, [_vp, _i32, _i64, _i32, _i32, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _i64, _i64,
                                       _vp]),
    "beast_logits_resident_rows": (_i64, [_i32, _i32, _i32, _vp]),
    "beast_xent_rows": (_i32, [_vp, _i32, _i64, _i32, _i32, _i64, _i64, _vp, _vp, _i64, _i64, _f32, _vp, _vp, _vp,
                               _vp]),
    "beast_xent_rows_bwd": (_i32, [_vp, _i32, _i64, _i32, _i32, _i64, _i64, _vp, _vp, _i64, _i64, _f32, _vp, _vp,
                                   _vp, _i64, _i64, _vp]),
    "beast_sample_rows": (_i32, [_vp, _i32, _i64, _i32, _i32, _i64, _i64, _f32, _i32, _f32, _vp, _i32, _i64, _vp, _vp,
                                 _vp, _vp]),
    "beast_score_rows": (_i32, [_vp, _i32, _i64, _i32, _i32, _i64, _i64, _vp, _i64, _i64, _f32, _i32, _f32, _vp, _i32,
                                _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "beast_score_rows_bwd": (_i32, [_vp, _i32, _i64, _i32, _i32, _i64, _i64, _vp, _i64, _i64, _f32, _i32, _f32, _vp,
                                    _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "beast_roundtrip_stats_f32": (_i32, [_vp, _i64, _i32, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp,
                                         _vp, _i32, _i64, _vp, _vp, _vp, _vp]),
    "beast_colminmax_workspace_bytes": (_sz, [_i64, _i32]),
    "beast_colminmax_f32": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _sz, _vp]),
    "beast_quantile_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "beast_quantile_prepare": (_i32, [_vp, _i64, _i32, _i64, _i64, _i32, _vp, _vp, _sz, _vp]),
    "beast_quantile_prepare_segments": (_i32, [_vp, _i32, _i64, _i64, _i32, _i64, _i32, _vp, _vp, _sz, _vp]),
    "beast_quantile_hist_ptr": (_vp, [_vp, _i32, _i32]),
    "beast_quantile_passes": (_i32, [_i32]),
    "beast_quantile_hist_count": (_i64, [_i32, _i32, _i32, _i32]),
    "beast_quantile_hist": (_i32, [_i32, _i64, _i32, _i32, _i32, _vp, _vp]),
    "beast_quantile_select": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp]),
    "beast_quantile_finalize": (_i32, [_i32, _i32, _vp, _vp, _vp]),
    "beast_quantile_f32": (_i32, [_vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _sz, _vp]),
    "beast_i64_minmax": (_i32, [_vp, _i64, _vp, _vp]),
    "beast_bpe_cp_presence": (_i32, [_vp, _i64, _i64, _vp, _i64, _vp]),
    "beast_bpe_pretok_count": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "beast_scan_workspace_bytes": (_sz, [_i64]),
    "beast_exclusive_scan_i64": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "beast_bpe_pretok_emit": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "beast_bpe_count_pairs": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _vp]),
    "beast_bpe_word_signatures": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "beast_bpe_argmax_workspace_bytes": (_sz, [_i32]),
    "beast_bpe_argmax": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp]),
    "beast_bpe_merge": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i64, _vp]),
    "beast_bpe_apply_argmax": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "beast_bpe_loop_workspace_bytes": (_sz, [_i32, _i32]),
    "beast_bpe_loop_init": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "beast_bpe_loop_state": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "beast_bpe_batch_workspace_bytes": (_sz, [_i32]),
    "beast_bpe_batch_delta_count": (_sz, [_i32]),
    "beast_bpe_loop_batch": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _vp,
                                    _vp, _vp, _sz, _i32, _vp, _vp, _vp]),
    "beast_bpe_dedup_workspace_bytes": (_sz, [_i64]),
    "beast_bpe_dedup_workspace_bytes_safe": (_sz, [_i64]),
    "beast_bpe_dedup_words": (_i32, [_vp, _vp, _vp, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "beast_bpe_repack_workspace_bytes": (_sz, [_i64]),
    "beast_bpe_pretok_dedup_workspace_bytes": (_sz, [_i64]),
    "beast_bpe_pretok_dedup": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _sz, _vp, _vp]),
    "beast_bpe_pretok_dedup_repack": (_i32, [_vp, _i64, _vp, _vp, _sz, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp,
                                             _vp]),
    "beast_bpe_repack_words": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "beast_bpe_compact_words": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "beast_bpe_mergemap_log2cap": (_i32, [_i32]),
    "beast_bpe_mergemap_bytes": (_sz, [_i32]),
    "beast_bpe_mergemap_build": (_i32, [_vp, _vp, _vp, _i32, _vp, _sz, _vp]),
    "beast_bpe_encode_lds_bytes": (_sz, [_i32, _i32]),
    "beast_bpe_encode_rows": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _i32,
                                     _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    "beast_bpe_train": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp,
                               _i32, _vp, _vp, _i32, _vp, _vp]),
    "beast_comm_id_bytes": (_sz, []),
    "beast_comm_unique_id": (_i32, [_vp]),
    "beast_comm_init_rank": (_i32, [_i32, _i32, _vp, _i32, _vp]),
    "beast_comm_init": (_i32, [_i32, _vp, _vp]),
    "beast_comm_init_virtual": (_i32, [_i32, _i32, _vp]),
    "beast_comm_group_start": (_i32, []),
    "beast_comm_group_end": (_i32, []),
    "beast_comm_destroy": (_i32, [_vp]),
    "beast_comm_info": (_i32, [_vp, _vp, _vp, _vp]),
    "beast_comm_allreduce": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "beast_comm_allgather": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "beast_comm_allgatherv": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "beast_bpe_train_comm": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp,
                                    _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "beast_bpe_wordmap_log2buckets": (_i32, [_i32]),
    "beast_bpe_wordmap_bytes": (_sz, [_i32]),
    "beast_bpe_wordmap_build_host": (_i32, [_vp, _vp, _vp, _i32, _vp, _sz, _vp]),
    "beast_bpe_encode_rows_words": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32,
                                           _i32, _vp, _i64, _vp, _vp, _vp]),
    "beast_bpe_decode_rows": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _vp, _vp, _vp, _vp]),
}

_lock = threading.Lock()
_lib: Optional[C.CDLL] = None


def load(path: str = LIB_PATH) -> C.CDLL:
    """dlopen the library and bind every symbol (no GPU needed)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise RuntimeError(
                f"libbeast_hip.so not found at {path}: build it with "
                "`python -m beast_tokenizer_amd._build` (there is no CPU fallback)")
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.beast_abi_version() != ABI_VERSION:
            raise RuntimeError("libbeast_hip.so ABI version mismatch; rebuild it")
        _lib = lib
        return lib


class BeastError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    if rc == BEAST_OK:
        return
    msg = (load().beast_last_error() or b"").decode(errors="replace")
    text = f"{what}: {msg}" if what else msg
    if rc == BEAST_E_INVALID:
        raise ValueError(text)
    if rc == BEAST_E_UNSUPPORTED:
        raise NotImplementedError(text)
    raise BeastError(text)


def call(name: str, *args) -> int:
    lib = load()
    rc = getattr(lib, name)(*args)
    return rc


def run(name: str, *args) -> None:
    """Call a status-returning entry point and raise on failure."""
    check(call(name, *args), name)


class CodecLaunch(NamedTuple):
    """Decoded BEAST_OPT_LAST_CODEC_LAUNCH (include/beast_hip.h): the kernel the last encode /
    reconstruct launch of this process chose."""
    family: Optional[str]   # one of CODEC_FAMILIES; None before any launch
    tile: int               # trajectories per tile
    waves: int              # waves per workgroup
    ks: int                 # MFMA K-steps over the basis functions (reconstruct)
    fast: bool              # encode input by contiguous DMA
    basis_regs: bool        # reconstruct basis operands in registers
    staged: bool            # output staged through LDS
    latency: bool           # latency variant (write-through stores) rather than the bulk one
    raw: int


def decode_codec_launch(v: int) -> CodecLaunch:
    fam = v & 15
    return CodecLaunch(CODEC_FAMILIES[fam] if fam < len(CODEC_FAMILIES) else None, (v >> 4) & 31, (v >> 9) & 31,
                       (v >> 14) & 7, bool(v >> 17 & 1), bool(v >> 18 & 1), bool(v >> 19 & 1), bool(v >> 20 & 1), v)


def last_codec_launch() -> CodecLaunch:
    """The kernel choice of this process's last encode / reconstruct launch (tests, tools)."""
    return decode_codec_launch(load().beast_get_option(OPT_LAST_CODEC_LAUNCH))


def last_launch_grid() -> int:
    """gridDim.x of this process's last kernel launch through the library, 0 before any (tests)."""
    return load().beast_get_option(OPT_LAST_LAUNCH_GRID)


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def raw_stream(index: int) -> int:
    """hipStream_t of the current stream of device ``index`` (cheap: no Stream object)."""
    return torch._C._cuda_getCurrentRawStream(index)


def stream_of(device: torch.device) -> int:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


def require_gpu(t: torch.Tensor, what: str = "tensor") -> None:
    if t.device.type != "cuda":
        raise RuntimeError(
            f"{what} is on {t.device}: the BEAST hot path runs only on a ROCm GPU "
            "(MI355X, gfx950); there is no CPU fallback")
    load()
