"""BEASTBsplineTokenizer -- drop-in for beast/beast_bspline_tokenizer.py:45-720.

Same constructor, attributes, methods, return types, on-disk format and error
types as the reference; every per-batch computation runs in libbeast_hip.so on a
ROCm GPU (MI355X / gfx950):

* ``encode``          -> ``beast_encode_f32``: fit + clamp + quantise + (d t)->(t d)
                         + LLM offset in one kernel (reference :399-428)
* ``encode_at``       -> ``beast_encode_rows_f32``: the same on per-trajectory time stamps with
                         sample weights (learn_mp_params_from_trajs with [B, T] times,
                         mp/uni_bspline.py:471-602); an extension of the surface
* ``compute_weights`` -> ``beast_encode_f32`` without the quantiser (:344-360)
* ``decode``          -> ``beast_reconstruct_f32`` dequantise only (:483-496)
* ``reconstruct_traj``-> ``beast_reconstruct_f32`` (:498-536)
* ``fit_parameters``  -> fit kernel + GPU radix-select quantiles (:181-220)

Tensors on the CPU are moved to ``self.device`` exactly as the reference does
(``trajs.to(self.device)``); a non-GPU device raises ``RuntimeError`` when
compute is requested (config / serialisation work anywhere).

Deliberate divergences:
* ``from_pretrained`` works: the reference passes ``tokenizer_type`` back into
  ``__init__`` and raises TypeError (:322, :333); here ``__init__`` accepts it.
* ``compute_reconstruction_error(..., return_tokens=True)`` (used by
  train/eval.py:34) is accepted.
* ``reconstruct_traj_continuous`` implements the intent of ``denormalize_tensor``
  (beast/utils.py:42 raises TypeError in the reference).
* ``init_cond_order`` / ``end_cond_order`` != 0 run the same fit kernel with the
  conditioned projection (``bspline.DeviceBasis``).  As the
  reference's MP object does, the last fit's boundary conditions are kept and reused
  by ``reconstruct_traj``.
"""
from __future__ import annotations

import json
import numbers
import struct
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .base_tokenizer import TokenizerBase
from .bspline import DeviceBasis, built

CONFIG_FILENAME = "beast_tokenizer_config.json"


def _tqdm(it, **kw):
    try:
        from tqdm import tqdm
        return tqdm(it, **kw)
    except Exception:  # pragma: no cover
        return it


class ReconstructionStats(NamedTuple):
    """What ``reconstruction_stats`` returns: device tensors, one row per trajectory and one
    column per output column (``[B, num_dof]`` fp32) unless noted."""
    mse: torch.Tensor                    # mean_t (raw - reconstructed)^2
    mean_err: torch.Tensor               # mean_t (raw - reconstructed), signed
    max_abs: torch.Tensor                # max_t |raw - reconstructed| (NaN propagates)
    mse_fit: Optional[torch.Tensor]      # mean_t (raw - spline fit)^2, before clamp / quantisation; None
                                         #   for tokenizers with init / end conditions
    clip_low: torch.Tensor               # int64 [num_dof, num_basis], w_min's (d n) order: trajectories
    clip_high: torch.Tensor              #   whose param lies below w_min / above w_max
    tokens: Optional[torch.Tensor]       # [B, num_basis*num_dof] as ``encode`` returns them, or None

    @property
    def l2(self) -> torch.Tensor:
        """Batch mean of ``mse``: ``compute_reconstruction_error``'s first value."""
        return self.mse.mean()

    @property
    def l1(self) -> torch.Tensor:
        """Batch mean of ``mean_err``: ``compute_reconstruction_error``'s second value."""
        return self.mean_err.mean()


class _MPInfo:
    """Lightweight stand-in for the reference's ``self.mp`` / ``self.gripper_mp``
    objects (mp_pytorch UniformBSpline): carries their configuration only."""

    def __init__(self, num_dof: int, num_basis: int, degree_p: int, tau: float):
        self.num_dof, self.num_basis, self.degree_p, self.tau = num_dof, num_basis, degree_p, tau

    def __repr__(self) -> str:
        return (f"UniformBSpline(num_dof={self.num_dof}, num_basis={self.num_basis}, degree_p={self.degree_p}, "
                f"tau={self.tau:.6g})")


def widen_bounds(w_min: torch.Tensor, w_max: torch.Tensor, batch_min: torch.Tensor, batch_max: torch.Tensor) -> None:
    """In place: take a batch extreme where it lies beyond the bound by more than 1e-4
    (reference beast_bspline_tokenizer.py:384-389: the masks, then ``masked_scatter_``; a
    ``where`` writes the same values).  Pure torch: the device-agnostic step after the
    (all-reduced) batch min/max."""
    wmin = w_min.to(batch_min.device)
    wmax = w_max.to(batch_max.device)
    smaller_mask = batch_min < (wmin - 1e-4)
    larger_mask = batch_max > (wmax + 1e-4)
    w_min.copy_(torch.where(smaller_mask, batch_min, wmin).to(w_min.device))
    w_max.copy_(torch.where(larger_mask, batch_max, wmax).to(w_max.device))


_FAST = None


def _fastpath():
    """The in-tree C++ host fast path (csrc/fastpath.cpp) if it was built from the current source
    (its .sha256 stamp matches), else None: a library built from an older fastpath.cpp may lack
    entry points the plan uses, so it is never loaded."""
    global _FAST
    if _FAST is None:
        _FAST = False
        from . import _build
        if _build.fastpath_current():
            import importlib.util
            so = _build.fastpath_so()
            spec = importlib.util.spec_from_file_location(_build.FAST_NAME, so)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            if all(hasattr(mod, f) for f in ("make_plan", "fast_encode", "fast_reconstruct")):
                _FAST = mod
    return _FAST or None


class _Plan:
    """Launch state of the hot path on one device: the cached constants (basis Phi,
    fp32 projection P, DoF maps) and the bound tensors, kept as raw pointers so a
    call costs two allocations and one C call.  Rebuilt when the time grid or the
    bound tensors change (in-place updates of ``w_min`` / ``w_max`` keep it valid)."""

    __slots__ = ("dev", "idx", "version", "wmin", "wmax", "keep", "T", "min_din", "dkey", "pinned",
                 "p_phi", "p_proj", "p_src", "p_dst", "p_wmn", "p_wmx", "enc", "rec", "fast", "fast_addr",
                 "fast_enc", "fast_rec", "llm", "off", "enc_win", "rec_win")

    def __init__(self, tok: "BEASTBsplineTokenizer", dev: torch.device):
        lib = _lib.load()
        phi, _, proj32 = tok._constants(dev)
        src, dst = tok._dof_maps(dev)
        wmn, wmx = tok._bounds(dev)
        self.dev, self.idx, self.version = dev, dev.index, tok._times_version
        self.dkey = tok.device                                  # the device argument it was built for
        self.pinned = torch.device(tok.device).index is not None
        self.wmin, self.wmax = tok.w_min, tok.w_max
        # the LLM-vocabulary offset the hot path adds (reference :456-481): part of the plan's key
        self.llm = tok.llm_vocab_size
        self.off = tok.llm_vocab_size - tok.vocab_size if tok.llm_vocab_size is not None else 0
        self.keep = (phi, proj32, src, dst, wmn, wmx)          # owns every pointer below
        self.T = phi.shape[1]
        order = tok.joint_indices + tok.gripper_indices
        self.min_din = (max(order) + 1) if order else 0
        self.p_phi, self.p_proj = phi.data_ptr(), proj32.data_ptr()
        self.p_src, self.p_dst = src.data_ptr(), dst.data_ptr()
        self.p_wmn, self.p_wmx = wmn.data_ptr(), wmx.data_ptr()
        self.enc, self.rec = lib.beast_encode_f32, lib.beast_reconstruct_f32
        self.enc_win = lib.beast_encode_windows_f32
        self.rec_win = lib.beast_reconstruct_windows_f32
        fp = _fastpath()
        self.fast = self.fast_addr = self.fast_enc = self.fast_rec = None
        if fp is not None and not tok._conditioned:
            import ctypes
            addr = lambda f: ctypes.cast(f, ctypes.c_void_p).value   # noqa: E731
            self.fast = fp.make_plan(addr(lib.beast_encode_f32), addr(lib.beast_reconstruct_f32),
                                     addr(lib.beast_last_error), dev.index, tok.num_dof, tok.joint_dof,
                                     tok.num_basis, self.T, tok.vocab_size, self.min_din, self.p_src, self.p_proj,
                                     self.p_wmn, self.p_wmx, self.p_phi, self.p_dst)
            # CPython fastcall entry points (csrc/fastpath.cpp): (plan address, tensor, offset);
            # self.fast keeps the plan they point at alive
            self.fast_addr = self.fast.addr()
            self.fast_enc, self.fast_rec = fp.fast_encode, fp.fast_reconstruct

    def cacheable(self) -> bool:
        # bounds living elsewhere were copied to the device: do not reuse the copy
        return self.keep[4] is self.wmin and self.keep[5] is self.wmax


class _ReconstructContinuous(torch.autograd.Function):
    """``reconstruct_traj_continuous`` (``orders`` None) / ``reconstruct_traj_continuous_derivs``
    with a backward.  The forward is the launch those methods always made; the backward is one
    launch of ``beast_reconstruct_derivs_bwd_f32`` over the slabs the forward used.  ``params`` is
    contiguous fp32 [B, N*D] on the plan's device, ``init_p`` what ``_init_p_rows`` returns."""

    @staticmethod
    def forward(ctx, params, init_p, tok, p, times, orders):
        B = params.shape[0]
        if orders is None:   # beast_reconstruct_f32: its [2][T][N] basis is order 0's slab
            basis = tok._basis_for(times, B, p)
            outs = (tok._reconstruct(None, params, times, init_p, False, p, basis),)
            keep, p_basis, basis_sb, slots = basis[0], basis[1], basis[2], (0,)
        else:
            basis = tok._deriv_basis_for(times, B, p, orders)
            outs = tok._reconstruct_derivs(None, params, times, orders, init_p, False, p, basis)
            keep, p_basis, basis_sb, slots = basis[0], basis[0].data_ptr(), basis[1], orders
        ctx.set_materialize_grads(False)       # an unused output's gradient stays None: a null pointer
        ctx.save_for_backward(params)
        # keep and p own the memory behind p_basis and the plan's pointers
        ctx.state = (tok, p, keep, p_basis, basis_sb, outs[0].shape[1], slots,
                     None if init_p is None else tuple(init_p.shape))
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        (params,) = ctx.saved_tensors
        tok, p, _, p_basis, basis_sb, Tn, slots, ip_shape = ctx.state
        none = (None,) * 6
        if all(g is None for g in grads):
            return none
        g3 = [None, None, None]
        for o, g in zip(slots, grads):
            if g is not None:   # y.sum().backward() delivers a stride-0 expansion: the kernel needs rows
                g3[o] = g.to(device=p.dev, dtype=torch.float32).contiguous()
        grad_params = torch.empty_like(params)
        grad_ip = None
        if ip_shape is not None and ctx.needs_input_grad[1]:
            grad_ip = torch.zeros(ip_shape, dtype=torch.float32, device=p.dev)
        _lib.run("beast_reconstruct_derivs_bwd_f32", *map(_lib.ptr, g3), params.shape[0], tok.num_dof, tok.joint_dof,
                 tok.num_basis, p.p_wmn, p.p_wmx, p_basis, basis_sb, Tn, p.p_dst, tok.num_dof, params.data_ptr(),
                 None if ip_shape is None else p.p_dst, grad_params.data_ptr(), _lib.ptr(grad_ip),
                 0 if ip_shape is None else ip_shape[1], _lib.raw_stream(p.idx))
        return (grad_params if ctx.needs_input_grad[0] else None, grad_ip) + none[2:]


def _logits_expect(logits, temperature, tok_offset, want_mean, want_tokens, want_stats):
    """One launch of ``beast_logits_expect`` on the current stream of the logits' device.
    ``logits`` is [B, K, V] fp32 / fp16 / bf16 on a ROCm device with unit last stride (any view: its
    strides go to the kernel).  Returns (mean, tokens, stats), None where not requested."""
    B, K, V = logits.shape
    dev = logits.device
    mean = torch.empty((B, K), dtype=torch.float32, device=dev) if want_mean else None
    tokens = torch.empty((B, K), dtype=torch.int64, device=dev) if want_tokens else None
    stats = torch.empty((B, K, 2), dtype=torch.float32, device=dev) if want_stats else None
    if B > 0:
        _lib.run("beast_logits_expect", logits.data_ptr(), _lib.LOGITS_DTYPES[logits.dtype], B, K, V,
                 logits.stride(0), logits.stride(1), temperature, tok_offset, _lib.ptr(mean), _lib.ptr(tokens),
                 _lib.ptr(stats), _lib.stream_of(dev))
    return mean, tokens, stats


class _ExpectedParams(torch.autograd.Function):
    """``expected_params_from_logits`` with a backward: one launch of ``beast_logits_expect`` (mean and
    the row statistics, the greedy tokens too when asked for) forward, one of ``beast_logits_expect_bwd``
    backward.  ``logits`` is what ``_logits_expect`` takes; the move, reshape, slice and cast that made
    it lie outside, so autograd carries the gradient back to the leaf's own shape, dtype and place."""

    @staticmethod
    def forward(ctx, logits, temperature, want_tokens):
        mean, tokens, stats = _logits_expect(logits, temperature, 0, True, want_tokens, True)
        ctx.save_for_backward(logits, mean, stats)
        ctx.temperature = temperature
        if tokens is None:
            return mean
        ctx.mark_non_differentiable(tokens)
        return mean, tokens

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mean, *_):
        logits, mean, stats = ctx.saved_tensors
        B, K, V = logits.shape
        dev = logits.device
        grad = torch.empty((B, K, V), dtype=logits.dtype, device=dev)
        if B > 0:
            g = grad_mean.to(device=dev, dtype=torch.float32).contiguous()   # a stride-0 expansion becomes rows
            _lib.run("beast_logits_expect_bwd", logits.data_ptr(), _lib.LOGITS_DTYPES[logits.dtype], B, K, V,
                     logits.stride(0), logits.stride(1), ctx.temperature, mean.data_ptr(), stats.data_ptr(),
                     g.data_ptr(), grad.data_ptr(), K * V, V, _lib.stream_of(dev))
        return grad, None, None


def _xent_targets(target):
    """(target_tok, target_pos) pointers of a [B, K] contiguous int64 or fp32 target."""
    return (target.data_ptr(), None) if target.dtype is torch.int64 else (None, target.data_ptr())


def _xent_rows(logits, target, tok_offset, ignore_index, smoothing, want_loss, want_tokens, want_stats):
    """One launch of ``beast_xent_rows`` on the current stream of the logits' device.  ``logits`` is
    what ``_logits_expect`` takes, ``target`` [B, K] contiguous int64 tokens or fp32 normalised
    coefficients on the same device.  Returns (loss, tokens, stats), None where not requested."""
    B, K, V = logits.shape
    dev = logits.device
    loss = torch.empty((B, K), dtype=torch.float32, device=dev) if want_loss else None
    tokens = torch.empty((B, K), dtype=torch.int64, device=dev) if want_tokens else None
    stats = torch.empty((B, K, 2), dtype=torch.float32, device=dev) if want_stats else None
    if B > 0:
        _lib.run("beast_xent_rows", logits.data_ptr(), _lib.LOGITS_DTYPES[logits.dtype], B, K, V,
                 logits.stride(0), logits.stride(1), *_xent_targets(target), tok_offset, ignore_index, smoothing,
                 _lib.ptr(loss), _lib.ptr(stats), _lib.ptr(tokens), _lib.stream_of(dev))
    return loss, tokens, stats


SAMPLE_MAX_DRAWS = 64      # beast_sample_rows: one draw per lane


def _sample_rows(logits, uniforms, temperature, top_k, top_p, tok_offset, want_logprob, want_kept=False):
    """One launch of ``beast_sample_rows`` on the current stream of the logits' device.  ``logits``
    is what ``_logits_expect`` takes, ``uniforms`` [S, B, K] contiguous fp32 on the same device.
    Returns (tokens [S, B, K], logprob or None, kept [B, K] or None)."""
    B, K, V = logits.shape
    S = uniforms.shape[0]
    dev = logits.device
    tokens = torch.empty((S, B, K), dtype=torch.int64, device=dev)
    logprob = torch.empty((S, B, K), dtype=torch.float32, device=dev) if want_logprob else None
    kept = torch.empty((B, K), dtype=torch.int32, device=dev) if want_kept else None
    if B > 0:
        _lib.run("beast_sample_rows", logits.data_ptr(), _lib.LOGITS_DTYPES[logits.dtype], B, K, V,
                 logits.stride(0), logits.stride(1), temperature, top_k, top_p, uniforms.data_ptr(), S, tok_offset,
                 tokens.data_ptr(), _lib.ptr(logprob), _lib.ptr(kept), _lib.stream_of(dev))
    return tokens, logprob, kept


class _CrossEntropy(torch.autograd.Function):
    """``cross_entropy_from_logits`` per row with a backward: one launch of ``beast_xent_rows`` (loss
    and the row statistics, the greedy tokens too when asked for) forward, one of
    ``beast_xent_rows_bwd`` backward.  As with ``_ExpectedParams`` the move, reshape, slice and cast
    that made ``logits`` lie outside; the target is never differentiable."""

    @staticmethod
    def forward(ctx, logits, target, tok_offset, ignore_index, smoothing, want_tokens):
        loss, tokens, stats = _xent_rows(logits, target, tok_offset, ignore_index, smoothing, True, want_tokens, True)
        ctx.save_for_backward(logits, target, stats)
        ctx.consts = (tok_offset, ignore_index, smoothing)
        if tokens is None:
            return loss
        ctx.mark_non_differentiable(tokens)
        return loss, tokens

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, *_):
        logits, target, stats = ctx.saved_tensors
        B, K, V = logits.shape
        dev = logits.device
        grad = torch.empty((B, K, V), dtype=logits.dtype, device=dev)
        if B > 0:
            g = grad_loss.to(device=dev, dtype=torch.float32).contiguous()   # a stride-0 expansion becomes rows
            _lib.run("beast_xent_rows_bwd", logits.data_ptr(), _lib.LOGITS_DTYPES[logits.dtype], B, K, V,
                     logits.stride(0), logits.stride(1), *_xent_targets(target), *ctx.consts, stats.data_ptr(),
                     g.data_ptr(), grad.data_ptr(), K * V, V, _lib.stream_of(dev))
        return grad, None, None, None, None, None


SCORE_STATS = 10           # beast_score_rows: floats per row of stats_out


def _score_rows(logits, ref, tokens, temperature, top_k, top_p, tok_offset, ignore_index, want_entropy, want_stats):
    """One launch of ``beast_score_rows`` on the current stream of the logits' device.  ``logits`` is
    what ``_logits_expect`` takes, ``ref`` None or a view of the same shape and dtype, ``tokens`` None
    or [S, B, K] contiguous int64 on the same device.  Returns (logprob [S, B, K], entropy [B, K],
    kl [B, K], stats), None where not requested."""
    B, K, V = logits.shape
    S = 0 if tokens is None else tokens.shape[0]
    dev = logits.device
    logprob = torch.empty((S, B, K), dtype=torch.float32, device=dev) if S else None
    entropy = torch.empty((B, K), dtype=torch.float32, device=dev) if want_entropy else None
    kl = torch.empty((B, K), dtype=torch.float32, device=dev) if ref is not None else None
    stats = torch.empty((B, K, SCORE_STATS), dtype=torch.float32, device=dev) if want_stats else None
    if B > 0:
        _lib.run("beast_score_rows", logits.data_ptr(), _lib.LOGITS_DTYPES[logits.dtype], B, K, V,
                 logits.stride(0), logits.stride(1), _lib.ptr(ref), ref.stride(0) if ref is not None else 0,
                 ref.stride(1) if ref is not None else 0, temperature, top_k, top_p, _lib.ptr(tokens), S, tok_offset,
                 ignore_index, _lib.ptr(logprob), _lib.ptr(entropy), _lib.ptr(kl), None, _lib.ptr(stats),
                 _lib.stream_of(dev))
    return logprob, entropy, kl, stats


class _ScoreTokens(torch.autograd.Function):
    """``score_tokens_from_logits`` with a backward: one launch of ``beast_score_rows`` forward (the
    log-probabilities, the entropy, the divergence and the row statistics), one of
    ``beast_score_rows_bwd`` backward for all three upstream gradients.  As with ``_CrossEntropy`` the
    move, reshape, slice and cast that made ``logits`` lie outside; the reference and the tokens are
    never differentiable.  Returns (logprob, entropy, kl) with empty tensors for the parts not asked
    for."""

    @staticmethod
    def forward(ctx, logits, ref, tokens, consts, want_entropy):
        logprob, entropy, kl, stats = _score_rows(logits, ref, tokens, *consts, want_entropy, True)
        ctx.save_for_backward(logits, stats, *(t for t in (ref, tokens) if t is not None))
        ctx.has = (ref is not None, tokens is not None, want_entropy)
        ctx.consts = consts
        empty = logits.new_empty(0, dtype=torch.float32)
        return tuple(empty if t is None else t for t in (logprob, entropy, kl))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_logprob, grad_entropy, grad_kl):
        logits, stats, *rest = ctx.saved_tensors
        has_ref, has_tokens, has_entropy = ctx.has
        ref = rest.pop(0) if has_ref else None
        tokens = rest.pop(0) if has_tokens else None
        B, K, V = logits.shape
        dev = logits.device
        grad = torch.empty((B, K, V), dtype=logits.dtype, device=dev)
        if B > 0:
            def rows(g, used):                                # a stride-0 expansion becomes rows
                return g.to(device=dev, dtype=torch.float32).contiguous() if used else None
            g_lp, g_h, g_kl = rows(grad_logprob, has_tokens), rows(grad_entropy, has_entropy), rows(grad_kl, has_ref)
            temperature, top_k, top_p, tok_offset, ignore_index = ctx.consts
            _lib.run("beast_score_rows_bwd", logits.data_ptr(), _lib.LOGITS_DTYPES[logits.dtype], B, K, V,
                     logits.stride(0), logits.stride(1), _lib.ptr(ref), ref.stride(0) if has_ref else 0,
                     ref.stride(1) if has_ref else 0, temperature, top_k, top_p, _lib.ptr(tokens),
                     tokens.shape[0] if has_tokens else 0, tok_offset, ignore_index, stats.data_ptr(),
                     _lib.ptr(g_lp), _lib.ptr(g_h), _lib.ptr(g_kl), grad.data_ptr(), K * V, V, _lib.stream_of(dev))
        return grad, None, None, None, None


def _window_index(episode_offsets, seq_len: int, *, stride: int = 1, pad: str = "edge"):
    """The window table of a dataset of episodes: CPU int64 ``(starts, ends, episode)``, one entry per
    training sample, for ``encode_windows``.

    ``episode_offsets`` [E + 1], non-decreasing (a host sequence or CPU tensor): episode ``e`` is
    frames ``off[e] .. off[e + 1] - 1`` of the flat buffer.  ``pad="edge"``: every start
    ``off[e] + k * stride < off[e + 1]`` is a window (ceil(L / stride) per episode of length L), and
    a window that reaches past the episode repeats its last frame -- LeRobot's padding rule.
    ``pad="valid"``: only starts with ``start + seq_len <= off[e + 1]`` ((L - seq_len) // stride + 1
    per episode, none if L < seq_len).  ``ends`` is the window's episode end ``off[e + 1]``.
    Vectorised: no loop over windows, no GPU."""
    off = torch.as_tensor(episode_offsets)
    if off.device.type != "cpu" or off.dim() != 1 or off.numel() < 1 or off.dtype.is_floating_point:
        raise ValueError("episode_offsets must be a host sequence of E + 1 integer frame offsets")
    off = off.to(torch.int64)
    if stride < 1 or seq_len < 1:
        raise ValueError(f"stride={stride} and seq_len={seq_len} must be >= 1")
    if pad not in ("edge", "valid"):
        raise ValueError(f"pad={pad!r} is not 'edge' or 'valid'")
    length = off[1:] - off[:-1]
    if bool((length < 0).any()) or int(off[0]) < 0:
        raise ValueError("episode_offsets must be non-negative and non-decreasing")
    if pad == "edge":
        n = (length + (stride - 1)) // stride
    else:
        n = torch.where(length >= seq_len, (length - seq_len) // stride + 1, torch.zeros_like(length))
    episode = torch.repeat_interleave(torch.arange(n.numel(), dtype=torch.int64), n)
    first = torch.cumsum(n, 0) - n                       # index of each episode's first window
    k = torch.arange(episode.numel(), dtype=torch.int64) - first[episode]
    starts = off[:-1][episode] + k * stride
    ends = off[1:][episode]
    return starts, ends, episode


class BEASTBsplineTokenizer(TokenizerBase):

    def __init__(self, num_dof=1, num_basis=10, duration=2 * torch.pi, seq_len=50, vocab_size=256,
                 degree_p=4, gripper_zero_order=False, gripper_indices=None,
                 init_cond_order=0, end_cond_order=0, init_pos=True,
                 use_bpe=False, device="cuda", llm_vocab_size: Optional[int] = None,
                 tokenizer_type: Optional[str] = None):
        super().__init__()

        self.dt = 0.01  # reference :53

        # reference :55-70
        if gripper_indices is None or not gripper_zero_order:
            gripper_indices = []
        self.gripper_indices = sorted(gripper_indices)
        if not gripper_zero_order or len(self.gripper_indices) == 0:
            self.gripper_dof = 0
        else:
            self.gripper_dof = len(self.gripper_indices)
        self.joint_dof = num_dof - self.gripper_dof
        all_indices = set(range(num_dof))
        self.joint_indices = sorted(list(all_indices - set(self.gripper_indices)))

        self.bspline_config = {
            "mp_type": "uni_bspline", "device": device, "num_dof": self.joint_dof, "tau": duration,
            "mp_args": {"num_basis": num_basis, "degree_p": degree_p, "init_condition_order": init_cond_order,
                        "end_condition_order": end_cond_order, "dt": 0.01},
        }
        self.init_pos = init_pos
        self.mp = _MPInfo(self.joint_dof, num_basis, degree_p, duration)
        self.gripper_mp = None
        if gripper_zero_order and self.gripper_dof > 0:
            self.gripper_mp_config = {"mp_type": "uni_bspline", "device": device, "num_dof": self.gripper_dof,
                                      "tau": duration, "mp_args": {"num_basis": num_basis, "degree_p": 0}}
            self.gripper_mp = _MPInfo(self.gripper_dof, num_basis, 0, duration)
            print(
                f"Gripper MP initialized with {num_basis} basis functions for "
                f"{self.gripper_dof} DOFs at indices {self.gripper_indices}"
            )

        self.device = device
        self.num_dof = self.joint_dof + self.gripper_dof
        self.num_basis = num_basis
        self.degree_p = degree_p
        self.vocab_size = vocab_size
        self.duration = duration
        self.seq_length = seq_len
        self.use_bpe = use_bpe

        self._basis = DeviceBasis(num_basis, degree_p, duration, self.gripper_mp is not None,
                                  init_cond_order=init_cond_order, end_cond_order=end_cond_order)
        # boundary conditions of the joint MP: the reference's MP object keeps the last fit's
        # init / end conditions and reuses them in get_traj_pos (uni_bspline.py:126-166)
        self._conditioned = self._basis.conditioned and self.joint_dof > 0
        self._cond_state = None
        self._full_basis = {}
        self._full_deriv = {}
        self._times_version = 0
        # tensor_linspace(0, duration, seq_len) == torch.linspace in fp32 (util_matrix.py:114-116)
        self.times = torch.linspace(0, duration, seq_len).to(device)

        dev = torch.device(device)
        buf_dev = dev if dev.type == "cuda" else torch.device("cpu")
        self.register_buffer("w_min", -0.02 * torch.ones((num_dof * num_basis), device=buf_dev))
        self.register_buffer("w_max", 0.02 * torch.ones((num_dof * num_basis), device=buf_dev))
        self.llm_vocab_size = None
        self._dof_cache = {}
        self._plans = {}
        self._plan_hot = None
        self._dev_of = {}

        self._config = {
            'tokenizer_type': 'beast_bspline',
            'num_dof': num_dof,
            'num_basis': num_basis,
            'duration': float(duration),
            'seq_len': seq_len,
            'vocab_size': vocab_size,
            'degree_p': degree_p,
            'gripper_zero_order': gripper_zero_order,
            'gripper_indices': list(self.gripper_indices),
            'init_cond_order': init_cond_order,
            'end_cond_order': end_cond_order,
            'init_pos': init_pos,
            'use_bpe': use_bpe,
            'device': device,
        }

        if llm_vocab_size is not None:
            self.set_llm_vocab_size(llm_vocab_size)

    # ===============================================
    #           - device plumbing -
    # ===============================================

    @property
    def times(self) -> torch.Tensor:
        return self._times

    @times.setter
    def times(self, value: torch.Tensor) -> None:
        self._times = value
        self._times_version = getattr(self, "_times_version", 0) + 1

    def _dev(self) -> torch.device:
        dev = self._dev_of.get(self.device)
        if dev is None:
            dev = torch.device(self.device)
            if dev.type != "cuda":
                raise RuntimeError(
                    f"BEASTBsplineTokenizer(device={self.device!r}): the BEAST hot path runs only on a ROCm GPU "
                    "(MI355X, gfx950); there is no CPU fallback")
            _lib.load()
            self._dev_of[self.device] = dev
        if dev.index is None:
            idx = torch.cuda.current_device()
            dev = self._dev_of.get(idx)
            if dev is None:
                dev = self._dev_of[idx] = torch.device("cuda", idx)
        return dev

    def _plan(self) -> _Plan:
        # hot path: plain attribute / dict lookups only (nn.Module.__getattr__ on the buffers
        # costs ~0.3 us each, a large part of a B=4096 call)
        p = self._plan_hot
        if p is not None:
            b = self._buffers
            if (p.version == self._times_version and p.wmin is b.get("w_min") and p.wmax is b.get("w_max")
                    and p.llm == self.llm_vocab_size and p.dkey is self.device
                    and (p.pinned or p.idx == torch.cuda.current_device())):
                return p
        dev = self._dev()
        p = self._plans.get(dev.index)
        if (p is None or p.version != self._times_version or p.wmin is not self.w_min or p.wmax is not self.w_max
                or p.llm != self.llm_vocab_size):
            p = _Plan(self, dev)
            if p.cacheable():
                built(dev)   # a cached plan's constants are complete before another stream can be handed them
                self._plans[dev.index] = p
        self._plan_hot = p if p.cacheable() else None
        return p

    def _constants(self, dev: torch.device):
        t = self.times.to(dev, dtype=torch.float32).reshape(-1)
        return self._basis.constants(t, self._times_version)

    def _dof_maps(self, dev: torch.device):
        hit = self._dof_cache.get(dev)
        if hit is None:
            order = self.joint_indices + self.gripper_indices
            src = torch.tensor(order, dtype=torch.int32, device=dev)
            hit = (src, src.clone())  # dof_src (encode) == dof_dst (reconstruct)
            built(dev)
            self._dof_cache[dev] = hit
        return hit

    def _bounds(self, dev: torch.device):
        return (self.w_min.to(dev, torch.float32).contiguous(), self.w_max.to(dev, torch.float32).contiguous())

    def _offset(self, respect_llm_vocab_size: bool) -> int:
        if respect_llm_vocab_size and self.llm_vocab_size is not None:
            return self._llm_vocab_offset()
        return 0

    def _fit(self, trajs: torch.Tensor, tokens_offset: Optional[int], p: _Plan):
        """Launch the fused fit (+ quantise) kernel. Returns (params, tokens or None)."""
        if trajs.device != p.dev or trajs.dtype is not torch.float32:
            trajs = trajs.to(p.dev, dtype=torch.float32)
        shape = trajs.shape
        if len(shape) != 3 or shape[1] != p.T:
            # learn_mp_params_from_trajs asserts trajs.shape[:-1] == times.shape (uni_bspline.py:487)
            raise AssertionError(f"trajectory shape {tuple(shape)} does not match [B, {p.T}, num_dof] time grid")
        B, T, Din = shape
        if Din < p.min_din:
            raise IndexError(f"index {p.min_din - 1} is out of bounds for dimension 2 with size {Din}")
        st = trajs.stride()
        if st[2] != 1 and B * T * Din:
            trajs = trajs.contiguous()
            st = trajs.stride()
        DN = self.num_dof * self.num_basis
        params = torch.empty((B, DN), dtype=torch.float32, device=p.dev)
        if tokens_offset is None:
            tokens, p_tok, p_wmn, p_wmx = None, None, None, None
        else:
            tokens = torch.empty((B, DN), dtype=torch.int64, device=p.dev)
            p_tok, p_wmn, p_wmx = tokens.data_ptr(), p.p_wmn, p.p_wmx
        rc = p.enc(trajs.data_ptr(), B, T, st[0], st[1], st[2], Din, self.num_dof, self.joint_dof, p.p_src,
                   p.p_proj, self.num_basis, p_wmn, p_wmx, self.vocab_size, tokens_offset or 0, params.data_ptr(),
                   p_tok, _lib.raw_stream(p.idx))
        if rc:
            _lib.check(rc, "beast_encode_f32")
        if self._conditioned:
            self._store_conditions(trajs, p)
        return params, tokens

    def _cond_consts(self, dev: torch.device):
        """(joint DoF map int32, time grid fp32, joint knot vector) on dev for csrc/cond.hip."""
        key = (dev, self._times_version)
        cache = getattr(self, "_cond_cache", {})
        c = cache.get(key)
        if c is None:
            c = (torch.tensor(self.joint_indices, dtype=torch.int32, device=dev),
                 self.times.to(dev, torch.float32).reshape(-1).contiguous(),
                 self._basis.knots(dev, 0).to(torch.float32).contiguous())
            built(dev)
            self._cond_cache = {key: c}
        return c

    def _store_conditions(self, trajs: torch.Tensor, p) -> None:
        """init / end conditions of the joint MP from this batch (uni_bspline.py:499-550), kept
        for the next reconstruct as the reference's MP object keeps them: one launch of
        k_cond_fixed (csrc/cond.hip) over trajs [B, T, D] (fp32 on the plan's device)."""
        jidx, t, kv = self._cond_consts(p.dev)
        B, T = trajs.shape[0], trajs.shape[1]
        dj, ic, ec = jidx.numel(), self._basis.ic, self._basis.ec

        def out(*shape):
            return torch.empty(shape, dtype=torch.float32, device=p.dev)
        ip = iv = ep = ev = p_init = p_end = None
        if ic:
            ip, iv, p_init = out(B, dj), out(B, dj), out(B, dj, ic)
        if ec:
            ep, ev, p_end = out(B, dj), out(B, dj), out(B, dj, abs(ec))
        st = trajs.stride()
        _lib.run("beast_cond_fixed_f32", trajs.data_ptr(), B, T, st[0], st[1], st[2], jidx.data_ptr(), dj,
                 t.data_ptr(), kv.data_ptr(), self._basis.degrees[0], self._basis.n_ctrl, float(self._basis.tau),
                 ic, ec, *map(_lib.ptr, (ip, iv, ep, ev, p_init, p_end)),
                 _lib.stream_of(p.dev))
        self._cond_state = {"B": B, "init_pos": ip, "init_vel": iv, "end_pos": ep, "end_vel": ev,
                            "params_init": p_init, "params_end": p_end}

    def _cond_dict(self) -> dict:
        st = self._cond_state if self._conditioned else None
        if st is None:
            return {"init_pos": None, "init_vel": None, "end_pos": None, "end_vel": None}
        return {k: st[k] for k in ("init_pos", "init_vel", "end_pos", "end_vel")}

    def _add_conditions(self, pos: torch.Tensor, times, B: int, dev: torch.device, order: int = 0) -> torch.Tensor:
        """pos[..., joints] += boundary control points' term + init_pos (get_traj_pos with the
        last fit's conditions, uni_bspline.py:126-166).  ``order`` 1 / 2: the same term of the
        order-th time derivative -- that order's full derivative basis, and zeros for init_pos
        (the constant offset differentiates away)."""
        st = self._cond_state
        if st is None:
            raise RuntimeError("reconstruct with init/end conditions needs the conditions of a previous "
                               "encode / compute_weights (the reference keeps them in its MP object)")
        if st["B"] != B:
            raise RuntimeError(f"Sizes of tensors must match except in dimension 2. Expected size {st['B']} "
                               f"but got size {B} (boundary conditions were fitted on a batch of {st['B']})")
        sdev = next(v.device for v in (st["init_pos"], st["end_pos"]) if v is not None)
        if sdev != dev:   # the kernel reads these raw pointers on dev: refuse as ATen's einsum did
            raise RuntimeError(f"Expected all tensors to be on the same device, but found at least two devices, "
                               f"{sdev} and {dev}! (boundary conditions were fitted on {sdev})")
        if times is None and order:
            key = (dev, self._times_version, order)
            full = self._full_deriv.get(key)
            if full is None:
                self._full_deriv = {k: v for k, v in self._full_deriv.items() if k[:2] == key[:2]}
                full = self._full_deriv[key] = self._basis.full_deriv_basis_at(self.times.to(dev).reshape(-1), order)
                built(dev)
        elif times is None:
            key = (dev, self._times_version)
            full = self._full_basis.get(key)
            if full is None:
                self._full_basis = {key: self._basis.full_basis_at(self.times.to(dev).reshape(-1))}
                full = self._full_basis[key]
                built(dev)
        elif order:
            full = self._basis.full_deriv_basis_at(times.to(dev, dtype=torch.float32), order).contiguous()
        else:   # [T] or per-row [B, T] grids -> [T, C] / [B, T, C]
            full = self._basis.full_basis_at(times.to(dev, dtype=torch.float32)).contiguous()
        if full.dim() not in (2, 3) or full.shape[-2] != pos.shape[1]:
            raise ValueError(f"times grid {tuple(full.shape[:-1])} does not match positions {tuple(pos.shape)}")
        jidx = self._cond_consts(dev)[0]
        _lib.run("beast_cond_add_f32", pos.data_ptr(), B, pos.shape[1], pos.shape[2], jidx.data_ptr(), jidx.numel(),
                 full.data_ptr(), 0 if full.dim() == 2 else full.shape[-2] * full.shape[-1], self._basis.n_ctrl,
                 self._basis.ic, self._basis.ec, _lib.ptr(st["params_init"]), _lib.ptr(st["params_end"]),
                 _lib.ptr(torch.zeros_like(st["init_pos"]) if order and st["init_pos"] is not None
                          else st["init_pos"]),
                 _lib.stream_of(dev))
        return pos

    # ===============================================
    #           - tokenizer preparation -
    # ===============================================

    def set_llm_vocab_size(self, llm_vocab_size: Optional[int]):
        """Specify the upstream LLM vocabulary size (reference :145-168)."""
        if llm_vocab_size is None:
            self.llm_vocab_size = None
            self._config.pop('llm_vocab_size', None)
            return
        if not isinstance(llm_vocab_size, numbers.Integral):
            raise TypeError("llm_vocab_size must be an integer or None")
        llm_vocab_size = int(llm_vocab_size)
        if llm_vocab_size < self.vocab_size:
            raise ValueError(
                "llm_vocab_size must be greater or equal to tokenizer vocab size"
            )
        self.llm_vocab_size = llm_vocab_size
        self._config['llm_vocab_size'] = llm_vocab_size

    def update_vlm_vocab_size(self, vlm_vocab_size):
        """Backward-compatible alias for :meth:`set_llm_vocab_size`."""
        self.set_llm_vocab_size(vlm_vocab_size)

    def _llm_vocab_offset(self) -> int:
        if self.llm_vocab_size is None:
            raise ValueError("LLM vocab size is not set.")
        return self.llm_vocab_size - self.vocab_size

    @torch.no_grad()
    def fit_parameters(self, dataloader, max_samples=None, verbose=True, *, process_group=None):
        """Fit w_min/w_max as the 1%/99% quantiles of the fitted params (reference :181-220).

        ``max_samples`` counts batches, as in the reference.  With
        ``process_group`` (torch.distributed, RCCL) every rank fits its own shard
        and the quantiles are those of the union of all ranks' params.
        """
        from .quantile import column_quantiles
        from .bpe_train import no_reduce, torch_dist_reducer

        dev = self._dev()
        params = []
        sample_limit = max_samples if max_samples is not None else float("inf")
        iterator = _tqdm(dataloader, total=max_samples, desc="precomputing weight normalizer of MP",
                         unit="batch") if verbose else dataloader
        sample_count = 0
        group = []   # device-resident batches of one shape, fitted together in one launch
        for batch in iterator:
            if "actions" not in batch:
                raise KeyError("Expected batch to contain an 'actions' entry.")
            # the host loop runs once per batch (245 at K4) and paces the grouped launches: a
            # full-width batch is used as is (the reference's [..., :num_dof] view costs ~1.4 us),
            # and a batch like the group's first (which passed _listable) joins it directly
            act_chunks = batch["actions"]
            if not (isinstance(act_chunks, torch.Tensor) and act_chunks.dim() and act_chunks.shape[-1] == self.num_dof):
                act_chunks = act_chunks[..., : self.num_dof]
            g0 = group[0] if group else None
            if (g0 is not None and isinstance(act_chunks, torch.Tensor) and act_chunks.shape == g0.shape
                    and act_chunks.dtype is g0.dtype and act_chunks.device == g0.device
                    and act_chunks.is_contiguous() and act_chunks.data_ptr() % 16 == 0) \
                    or self._listable(act_chunks, group):
                group.append(act_chunks)
                if len(group) * act_chunks.shape[0] >= self._FIT_GROUP_ROWS:
                    params.append(self._fit_list(group))
                    group = []
            else:
                if group:
                    params.append(self._fit_list(group))
                    group = []
                params.append(self.compute_weights(act_chunks))
            sample_count += 1
            if sample_count >= sample_limit:
                if verbose:
                    print("Precomputed enough samples for weight normalizer of MP")
                break
        if group:
            params.append(self._fit_list(group))
        if not params and process_group is None:
            raise RuntimeError("No parameters were gathered from the dataloader.")
        # per-batch params are read in place by the quantile kernels (no concatenation)
        allp = params if params else torch.empty((0, self.num_dof * self.num_basis), device=dev)
        reduce = no_reduce if process_group is None else torch_dist_reducer(
            None if process_group is True else process_group)
        q = column_quantiles(allp, [0.01, 0.99], reduce)
        self.w_min.copy_(q[0].to(self.w_min.device))
        self.w_max.copy_(q[1].to(self.w_max.device))

    # ===============================================
    #           - tokenizer serialization -
    # ===============================================

    def get_config(self):
        config = self._config.copy()
        if self.llm_vocab_size is not None:
            config['llm_vocab_size'] = self.llm_vocab_size
        return config

    def state_dict(self):
        """Config + fitted bounds as JSON-able lists (reference :235-245)."""
        return {
            'config': self.get_config(),
            'w_min': self.w_min.cpu().numpy().tolist(),
            'w_max': self.w_max.cpu().numpy().tolist(),
            'llm_vocab_size': self.llm_vocab_size,
        }

    def load_state_dict(self, state_dict):
        """Reference :248-269."""
        if 'w_min' in state_dict:
            w_min = torch.tensor(state_dict['w_min'], dtype=torch.float32, device=self.w_min.device)
            self.w_min.copy_(w_min)
        if 'w_max' in state_dict:
            w_max = torch.tensor(state_dict['w_max'], dtype=torch.float32, device=self.w_max.device)
            self.w_max.copy_(w_max)
        llm_size = state_dict.get('llm_vocab_size')
        if llm_size is None:
            llm_size = state_dict.get('vlm_vocab_size')
        if llm_size is not None:
            self.set_llm_vocab_size(llm_size)
        print(f"✓ Loaded fitted parameters (w_min, w_max) with shape {self.w_min.shape}")

    def save_pretrained(self, save_directory):
        """Write ``beast_tokenizer_config.json`` (reference :272-290)."""
        save_directory = Path(save_directory)
        save_directory.mkdir(parents=True, exist_ok=True)
        state = self.state_dict()
        config_path = save_directory / CONFIG_FILENAME
        with open(config_path, 'w') as f:
            json.dump(state, f, indent=2)
        print(f"✓ Saved tokenizer to {save_directory}")
        print(f"  - Config: {config_path}")

    @classmethod
    def from_pretrained(cls, pretrained_path, device=None):
        """Reference :293-338 (works: ``tokenizer_type`` is accepted by ``__init__``)."""
        pretrained_path = Path(pretrained_path)
        config_path = pretrained_path / CONFIG_FILENAME
        if not config_path.exists():
            raise FileNotFoundError(f"Config file not found: {config_path}")
        with open(config_path, 'r') as f:
            state = json.load(f)
        config = state['config'].copy()
        tokenizer_type = config.get('tokenizer_type')
        if tokenizer_type not in {'beast_bspline', None}:
            raise ValueError(
                "Loaded configuration does not describe a BEAST B-Spline tokenizer."
            )
        config['tokenizer_type'] = 'beast_bspline'
        if device is not None:
            config['device'] = device
        print(f"✓ Loading tokenizer from {pretrained_path}")
        print(f"  - Config: num_dof={config['num_dof']}, num_basis={config['num_basis']}, "
              f"gripper_indices={config['gripper_indices']}")
        tokenizer = cls(**config)
        tokenizer.load_state_dict(state)
        return tokenizer

    # ===============================================
    #              - tokenizer utils -
    # ===============================================

    _FIT_GROUP_ROWS = 1 << 18   # rows per grouped fit launch (HBM-bound from ~64 k rows)

    def _listable(self, x, group) -> bool:
        """Can batch ``x`` join ``group`` for one beast_encode_list_f32 launch?  Device-resident
        contiguous fp32 [B, T, D] with B % 8 == 0 and 16-byte aligned rows, all of one shape
        (anything else takes the per-batch path)."""
        if not isinstance(x, torch.Tensor) or self._conditioned or x.dim() != 3:
            return False
        p = self._plan()
        if (x.device != p.dev or x.dtype is not torch.float32 or not x.is_contiguous() or x.shape[0] == 0
                or x.shape[0] % 8 or x.shape[1] != p.T or x.shape[2] < p.min_din or x.data_ptr() % 16
                or (x.shape[1] * x.shape[2]) % 4):
            return False
        return not group or group[0].shape == x.shape

    def _fit_list(self, group) -> torch.Tensor:
        """Params of a group of batches by one launch (bitwise the per-batch params)."""
        p = self._plan()
        if len(group) == 1:
            return self.compute_weights(group[0])
        B, T, Din = group[0].shape
        if any(g.shape != group[0].shape for g in group):   # the launch reads B rows from every pointer
            raise ValueError("_fit_list: every batch of a group must have the same shape")
        ptrs = torch.tensor([g.data_ptr() for g in group], dtype=torch.int64).pin_memory()
        ptrs = ptrs.to(p.dev, non_blocking=True)
        out = torch.empty((len(group) * B, self.num_dof * self.num_basis), dtype=torch.float32, device=p.dev)
        _lib.run("beast_encode_list_f32", ptrs.data_ptr(), len(group), B, T, Din, self.num_dof, self.joint_dof,
                 p.p_src, p.p_proj, self.num_basis, out.data_ptr(), _lib.raw_stream(p.idx))
        # the pointer table and the batches may be freed after this: the caching allocators
        # reuse their memory only in the order of the current stream (pinned: after the copy)
        return out

    @torch.no_grad()
    def compute_weights(self, demos):
        """Fitted params [B, num_dof*num_basis] in (d n) order (reference :344-360)."""
        p = self._plan()
        if p.fast is not None:
            r = p.fast.fit(demos, torch._C._cuda_getCurrentRawStream(p.idx))
            if r is not None:
                return r
        params, _ = self._fit(demos, None, p)
        return params

    def _batch_minmax(self, weights, process_group, active=True):
        """Column (min, max) of ``weights`` [rows, D*N] on this rank, all-reduced over
        ``process_group`` (None: this process only; True: the default group) so every rank
        holds the extremes of the global batch.  ``weights=None`` (or
        ``active=False``) takes part in the collective without rows.  Returns
        (mn, mx, any_rank_active)."""
        from .quantile import allreduce_minmax, column_minmax
        from .bpe_train import no_reduce, torch_dist_reducer
        cols = self.num_dof * self.num_basis
        if weights is not None and active:
            mn, mx = column_minmax(weights.reshape(-1, cols))
        else:
            if process_group is None:
                raise ValueError("an empty bounds update needs a process_group")
            dev = self._dev()
            mn = torch.full((cols,), float("inf"), dtype=torch.float32, device=dev)
            mx = torch.full((cols,), float("-inf"), dtype=torch.float32, device=dev)
            active = False
        reduce = no_reduce if process_group is None else torch_dist_reducer(
            None if process_group is True else process_group)
        return allreduce_minmax(mn, mx, reduce, active)

    @torch.no_grad()
    def update_weights_bounds(self, demos, *, process_group=None):
        """w_min/w_max <- column min/max of the batch's params (reference :362-378).
        ``process_group`` (extension, a collective): the min/max of every rank's batch."""
        weights = self.compute_weights(demos)
        mn, mx, _ = self._batch_minmax(weights, process_group)
        self.w_min.copy_(mn.to(self.w_min.device))
        self.w_max.copy_(mx.to(self.w_max.device))

    @torch.no_grad()
    def update_weights_bounds_per_batch(self, weights, *, process_group=None):
        """Widen w_min/w_max by the batch extremes beyond a 1e-4 margin (reference :379-389).
        ``process_group`` (extension, a collective): the extremes of the global batch, so
        every rank's bounds stay identical.  ``weights=None``: this rank has no batch this
        step but takes part; returns whether any rank had one (a 0-d bool tensor)."""
        batch_min, batch_max, any_active = self._batch_minmax(weights, process_group, weights is not None)
        widen_bounds(self.w_min, self.w_max, batch_min, batch_max)
        return any_active

    def update_times(self, times):
        self.times = times.to(self.device)

    # ===============================================
    #           - tokenizer encoding -
    # ===============================================

    def encode(self, trajs, update_bounds=False, *, respect_llm_vocab_size=True, process_group=None):
        """(tokens int64 [B, num_basis*num_dof], params_dict) -- reference :399-428.

        No autograd graph is recorded: the outputs are written by the kernel into fresh
        tensors (the reference runs under ``torch.no_grad`` equivalently).
        ``process_group`` (extension): with ``update_bounds`` the bounds widen by the
        extremes of every rank's batch (one all-reduce; a collective call), so all ranks
        quantise with the same bounds -- those of one process encoding the global batch."""
        p = self._plan()
        if not update_bounds and p.fast_enc is not None:
            # (tokens, {"params": ..., conditions None}); the plan carries the LLM offset
            r = p.fast_enc(p.fast_addr, trajs, p.off if respect_llm_vocab_size else 0)
            if r is not None:
                return r
        offset = p.off if respect_llm_vocab_size else 0
        if update_bounds:
            with torch.no_grad():
                params, _ = self._fit(trajs, None, p)
                self.update_weights_bounds_per_batch(params, process_group=process_group)
                tokens = self._quantize(params, offset, p.dev, mode=0)
        else:
            params, tokens = self._fit(trajs, offset, p)
        return tokens, {"params": params, **self._cond_dict()}

    def _quantize(self, params: torch.Tensor, offset: int, dev: torch.device, mode: int):
        B = params.shape[0]
        D, N = self.num_dof, self.num_basis
        wmn, wmx = self._bounds(dev)
        params = params.contiguous()
        if mode == 0:
            out = torch.empty((B, N * D), dtype=torch.int64, device=dev)
            _lib.run("beast_quantize_f32", params.data_ptr(), B, D, N, wmn.data_ptr(), wmx.data_ptr(),
                     self.vocab_size, offset, 0, out.data_ptr(), None, _lib.stream_of(dev))
        else:
            out = torch.empty((B, N * D), dtype=torch.float32, device=dev)
            _lib.run("beast_quantize_f32", params.data_ptr(), B, D, N, wmn.data_ptr(), wmx.data_ptr(),
                     self.vocab_size, 0, 1, None, out.data_ptr(), _lib.stream_of(dev))
        return out

    @torch.no_grad()
    def encode_continuous(self, trajs, update_bounds=False, *, process_group=None):
        """Normalised params in [-1, 1], (t d) order (reference :430-450)."""
        p = self._plan()
        params, _ = self._fit(trajs, None, p)
        if update_bounds:
            self.update_weights_bounds_per_batch(params, process_group=process_group)
        tokens = self._quantize(params, 0, p.dev, mode=1)
        params_dict = {"params": params, **self._cond_dict()}
        return tokens, params_dict

    # ===============================================
    #     - encoding on per-trajectory time grids -
    # ===============================================

    def _fit_rows(self, trajs, times, weights, tokens_offset: Optional[int]):
        """One launch of beast_encode_rows_f32 (csrc/fit_rows.hip): the weighted ridge fit of every
        trajectory on its own time stamps.  Returns (params, tokens or None, device).  The
        argument checks run before the device is asked for."""
        if self._basis.conditioned:
            raise NotImplementedError(
                "encode_at supports init_cond_order = end_cond_order = 0 only: the conditions come from "
                "y0, y1 and one dt of the shared grid (uni_bspline.py:499-550), not from per-row times")
        trajs, times = torch.as_tensor(trajs), torch.as_tensor(times)
        if trajs.dim() != 3 or times.dim() not in (1, 2) or tuple(times.shape) not in (
                tuple(trajs.shape[1:2]), tuple(trajs.shape[:2])):
            # learn_mp_params_from_trajs asserts trajs.shape[:-1] == times.shape (uni_bspline.py:487)
            raise AssertionError(f"trajectory shape {tuple(trajs.shape)} does not match times {tuple(times.shape)}: "
                                 "need [B, T, num_dof] with times [B, T] or [T]")
        B, T, Din = trajs.shape
        if T < 1:
            raise ValueError("times must hold at least one point")
        if weights is not None:
            weights = torch.as_tensor(weights)
            if weights.dim() not in (1, 2) or tuple(weights.shape) not in ((T,), (B, T)):
                raise ValueError(f"weights must be [T] or [B, T]; got {tuple(weights.shape)} for B={B}, T={T}")
        order = self.joint_indices + self.gripper_indices
        if order and Din <= max(order):
            raise IndexError(f"index {max(order)} is out of bounds for dimension 2 with size {Din}")
        dev = self._dev()

        def rows(x):   # fp32 on dev with unit stride along T; (tensor, batch stride)
            x = x.to(dev, dtype=torch.float32)
            if x.stride(-1) != 1 and T > 1:
                x = x.contiguous()
            return x, (x.stride(0) if x.dim() == 2 and B > 1 else 0)

        trajs = trajs.to(dev, dtype=torch.float32)
        times, t_sb = rows(times)
        w_sb = 0
        if weights is not None:
            weights, w_sb = rows(weights)
        D, N, basis = self.num_dof, self.num_basis, self._basis
        kj = basis.knots(dev, 0)
        kg = basis.knots(dev, 1) if basis.has_gripper else None
        src, _ = self._dof_maps(dev)
        params = torch.empty((B, D * N), dtype=torch.float32, device=dev)
        tokens = wmn = wmx = None
        if tokens_offset is not None:
            tokens = torch.empty((B, N * D), dtype=torch.int64, device=dev)
            wmn, wmx = self._bounds(dev)
        if B == 0:   # an empty tensor has no address to pass
            return params, tokens, dev
        st = trajs.stride()
        _lib.run("beast_encode_rows_f32", trajs.data_ptr(), B, T, st[0], st[1], st[2], D, self.joint_dof,
                 src.data_ptr(), times.data_ptr(), t_sb, _lib.ptr(weights), w_sb, basis.tau, basis.delay,
                 kj.data_ptr(), kj.numel(), _lib.ptr(kg), 0 if kg is None else kg.numel(), basis.degrees[0], N,
                 basis.reg, _lib.ptr(wmn), _lib.ptr(wmx), self.vocab_size, tokens_offset or 0, params.data_ptr(),
                 _lib.ptr(tokens), _lib.stream_of(dev))
        return params, tokens, dev

    @torch.no_grad()
    def encode_at(self, trajs, times, weights=None, update_bounds=False, *, respect_llm_vocab_size=True,
                  process_group=None):
        """``encode`` for trajectories on their OWN time stamps: (tokens int64 [B, num_basis*num_dof],
        {"params": fp32 [B, num_dof*num_basis], ...}) from one launch of ``beast_encode_rows_f32``.

        ``trajs`` [B, T, >= num_dof]; ``times`` [B, T] or [T] (seconds on the tokenizer's
        [0, duration] axis; T is the trajectory's own length and need not equal ``seq_len``);
        ``weights`` [B, T], [T] or None (all ones), >= 0.  Every trajectory gets the weighted ridge
        fit argmin sum_t w_t (y_t - Phi(t_t) p)^2 + reg |p|^2 of
        UniformBSpline.learn_mp_params_from_trajs (mp/uni_bspline.py:471-602) on its own basis, in
        float64, rounded once.  A weight of 0 skips the sample: its time and values are never
        read into the fit and may be NaN (missing frames, padded tails); a trajectory with no
        weight at all gets params 0.  Negative or non-finite weights are undefined.

        ``update_bounds`` / ``process_group`` / ``respect_llm_vocab_size`` as in ``encode``.
        Tokenizers with init / end conditions raise ``NotImplementedError``."""
        offset = self._offset(respect_llm_vocab_size)
        if update_bounds:
            params, _, dev = self._fit_rows(trajs, times, weights, None)
            self.update_weights_bounds_per_batch(params, process_group=process_group)
            tokens = self._quantize(params, offset, dev, mode=0)
        else:
            params, tokens, _ = self._fit_rows(trajs, times, weights, offset)
        return tokens, {"params": params, **self._cond_dict()}

    @torch.no_grad()
    def encode_continuous_at(self, trajs, times, weights=None, update_bounds=False, *, process_group=None):
        """``encode_continuous`` on per-trajectory time stamps: the params of ``encode_at``
        normalised to [-1, 1] in (t d) order."""
        params, _, dev = self._fit_rows(trajs, times, weights, None)
        if update_bounds:
            self.update_weights_bounds_per_batch(params, process_group=process_group)
        tokens = self._quantize(params, 0, dev, mode=1)
        return tokens, {"params": params, **self._cond_dict()}

    # ===============================================
    #     - encoding windows of an episode buffer -
    # ===============================================

    def window_index(self, episode_offsets, *, stride=1, pad="edge"):
        """The window table of a dataset of episodes for ``encode_windows``: CPU int64
        ``(starts, ends, episode)``, one entry per training sample of ``seq_len`` steps
        (``pad="edge"``: every start inside an episode, the last frame repeated past its end;
        ``pad="valid"``: whole windows only).  Vectorised, no GPU."""
        return _window_index(episode_offsets, int(self.times.numel()), stride=stride, pad=pad)

    def _fit_windows(self, frames, starts, ends, tokens_offset: Optional[int], want_counts: bool = False):
        """One launch of beast_encode_windows_f32 (csrc/windows.hip).  Returns (params, tokens or
        None, valid, tile counts or None, device).  The argument checks run before the device is
        asked for."""
        if self._basis.conditioned:
            raise NotImplementedError(
                "encode_windows supports init_cond_order = end_cond_order = 0 only: the conditions are kept "
                "per batch from y0, y1 of materialised trajectories (uni_bspline.py:499-550), and a window "
                "table has none")
        if not isinstance(frames, torch.Tensor):
            frames = torch.as_tensor(frames)
        if frames.dim() != 2:
            raise ValueError(f"frames must be [R, num_dof] (a flat frame buffer); got {tuple(frames.shape)}")
        R, Din = frames.shape
        min_din = max(self.joint_indices + self.gripper_indices, default=-1) + 1
        if Din < min_din:
            raise IndexError(f"index {min_din - 1} is out of bounds for dimension 1 with size {Din}")
        if not isinstance(starts, torch.Tensor):
            starts = torch.as_tensor(starts)
        if not isinstance(ends, torch.Tensor):
            ends = torch.as_tensor(ends)
        if (starts.dim() != 1 or starts.shape != ends.shape or starts.dtype is not torch.int64
                or ends.dtype is not torch.int64):
            raise ValueError(f"starts / ends must be int64 [W] tables of one length; got {tuple(starts.shape)} "
                             f"{starts.dtype} and {tuple(ends.shape)} {ends.dtype}")
        W = starts.shape[0]
        # host tables are checked here; a device table is not synchronised on (the kernel clamps it)
        if W and starts.device.type == "cpu" and ends.device.type == "cpu":
            if bool(((starts < 0) | (starts >= ends) | (ends > R)).any()):
                raise ValueError(f"window table out of range: need 0 <= start < end <= R={R} for every window")
        p = self._plan()
        dev, T = p.dev, p.T
        # the hot path (device-resident fp32 frames and tables) pays for no torch call it does not need
        if frames.device != dev or frames.dtype is not torch.float32:
            frames = frames.to(dev, dtype=torch.float32)
        st = frames.stride()
        if R and (st[1] != 1 or (R > 1 and st[0] < Din)):
            frames = frames.contiguous()
            st = frames.stride()
        if starts.device != dev:
            starts = starts.to(dev)
        if ends.device != dev:
            ends = ends.to(dev)
        if W > 1 and starts.stride(0) != 1:
            starts = starts.contiguous()
        if W > 1 and ends.stride(0) != 1:
            ends = ends.contiguous()
        DN = self.num_dof * self.num_basis
        params = torch.empty((W, DN), dtype=torch.float32, device=dev)
        tokens = p_tok = p_wmn = p_wmx = None
        if tokens_offset is not None:
            tokens = torch.empty((W, DN), dtype=torch.int64, device=dev)
            p_tok, p_wmn, p_wmx = tokens.data_ptr(), p.p_wmn, p.p_wmx
        # min(T, end - start): the subtraction lands in int32 (two launches in all)
        valid = torch.empty((W,), dtype=torch.int32, device=dev)
        torch.sub(ends, starts, out=valid).clamp_(max=T)
        counts = torch.zeros(2, dtype=torch.int32, device=dev) if want_counts else None
        if W:   # an empty tensor has no address to pass
            rc = p.enc_win(frames.data_ptr(), R, st[0], st[1], Din, starts.data_ptr(), ends.data_ptr(), W, T,
                           self.num_dof, self.joint_dof, p.p_src, p.p_proj, self.num_basis, p_wmn, p_wmx,
                           self.vocab_size, tokens_offset or 0, params.data_ptr(), p_tok,
                           None if counts is None else counts.data_ptr(), _lib.raw_stream(p.idx))
            if rc:
                _lib.check(rc, "beast_encode_windows_f32")
        return params, tokens, valid, counts, dev

    @torch.no_grad()
    def encode_windows(self, frames, starts, ends, update_bounds=False, *, respect_llm_vocab_size=True,
                       process_group=None, return_tile_counts=False):
        """``encode`` of the windows of a flat frame buffer, without materialising them: (tokens int64
        [W, num_basis*num_dof], {"params": fp32 [W, num_dof*num_basis], "valid": int32 [W], ...}) from
        one launch of ``beast_encode_windows_f32``.

        ``frames`` [R, >= num_dof], any row stride: every episode's frames, one after another.
        ``starts`` / ``ends`` int64 [W], on the host or the device (:meth:`window_index` builds them
        from episode offsets): window ``w`` is the trajectory ``frames[min(starts[w] + t, ends[w] - 1)]``
        for ``t < seq_len`` -- the next ``seq_len`` actions, the episode's last frame repeated past its
        end (LeRobot's padding rule).  Tokens and params are bitwise those of ``encode`` on the gathered
        [W, seq_len, D] tensor; ``valid`` is ``min(seq_len, end - start)``, the samples that are no
        padding.  Host tables are range-checked (``ValueError``); device tables are not read back:
        the kernel clamps them into the buffer, so a bad one gives wrong numbers, never a fault
        -- and ``valid`` is then ``min(seq_len, end - start)`` of the table AS GIVEN (it may be
        negative, or differ from the rows the kernel used after its clamp).

        ``update_bounds`` / ``process_group`` / ``respect_llm_vocab_size`` as in ``encode``.
        ``return_tile_counts`` adds ``"tile_counts"``: int32 [2], the kernel's tiles that shared one
        staged segment / that were gathered window by window.  Tokenizers with init / end conditions
        raise ``NotImplementedError``."""
        offset = self._offset(respect_llm_vocab_size)
        if update_bounds:
            params, _, valid, counts, dev = self._fit_windows(frames, starts, ends, None, return_tile_counts)
            self.update_weights_bounds_per_batch(params, process_group=process_group)
            tokens = self._quantize(params, offset, dev, mode=0)
        else:
            params, tokens, valid, counts, _ = self._fit_windows(frames, starts, ends, offset, return_tile_counts)
        info = {"params": params, "valid": valid, **self._cond_dict()}
        if return_tile_counts:
            info["tile_counts"] = counts
        return tokens, info

    @torch.no_grad()
    def encode_continuous_windows(self, frames, starts, ends, update_bounds=False, *, process_group=None):
        """``encode_continuous`` of the windows of a frame buffer: the params of ``encode_windows``
        normalised to [-1, 1] in (t d) order."""
        params, _, valid, _, dev = self._fit_windows(frames, starts, ends, None)
        if update_bounds:
            self.update_weights_bounds_per_batch(params, process_group=process_group)
        tokens = self._quantize(params, 0, dev, mode=1)
        return tokens, {"params": params, "valid": valid, **self._cond_dict()}

    @torch.no_grad()
    def fit_parameters_windows(self, frames, starts, ends, *, chunk_windows=1 << 20, process_group=None):
        """``fit_parameters`` over the windows of a frame buffer: w_min / w_max become the 1 % / 99 %
        quantiles of every window's fitted params.  The table is fitted ``chunk_windows`` windows at
        a time and the quantile kernels read the chunks' params in place.  With ``process_group``
        every rank fits its own table and the quantiles are those of the union."""
        from .quantile import column_quantiles
        from .bpe_train import no_reduce, torch_dist_reducer

        if chunk_windows < 1:
            raise ValueError("chunk_windows must be >= 1")
        starts, ends = torch.as_tensor(starts), torch.as_tensor(ends)
        if starts.dim() != 1 or ends.dim() != 1:
            self._fit_windows(frames, starts, ends, None)   # raises: the tables' shape
        W = starts.shape[0]
        params = []
        for i in range(0, max(W, 1), chunk_windows):
            pr = self._fit_windows(frames, starts[i:i + chunk_windows], ends[i:i + chunk_windows], None)[0]
            if pr.shape[0]:
                params.append(pr)
        if not params and process_group is None:
            raise RuntimeError("No parameters were gathered: the window table is empty.")
        allp = params if params else torch.empty((0, self.num_dof * self.num_basis), device=self._dev())
        reduce = no_reduce if process_group is None else torch_dist_reducer(
            None if process_group is True else process_group)
        q = column_quantiles(allp, [0.01, 0.99], reduce)
        self.w_min.copy_(q[0].to(self.w_min.device))
        self.w_max.copy_(q[1].to(self.w_max.device))

    # ===============================================
    #   - blending window tokens back into frames -
    # ===============================================

    def blend_weights(self, kind="uniform", *, m=0.01, horizon=None):
        """Blend weights for ``reconstruct_windows``: fp32 [seq_len] on the tokenizer's device, entry
        ``t`` the weight of a window's sample ``t`` (the row ``t`` frames after the window's start).

        ``"uniform"``: all ones, the plain mean of every chunk that covers a frame.
        ``"exp"``: ``exp(m * (t - (seq_len - 1)))``.  On a stride-1 table the chunks covering a frame
        are the ones predicted 0 .. seq_len-1 frames earlier and the oldest has the largest ``t``, so
        after the normalisation this is ACT's temporal ensembling ``exp(-m * i)`` with ``i = 0`` the
        oldest prediction; ``m > 0`` favours older chunks.  At table stride ``s`` consecutive chunks
        are ``s`` samples apart, so ACT's ``m`` corresponds to ``m / s`` here.
        ``"first"``: 1 for ``t < horizon``, else 0 -- the receding-horizon rule that executes the
        first ``horizon`` steps of each chunk."""
        T = int(self.times.numel())
        t = torch.arange(T, dtype=torch.float64)
        if kind == "uniform":
            w = torch.ones(T, dtype=torch.float64)
        elif kind == "exp":
            w = torch.exp(float(m) * (t - (T - 1)))
        elif kind == "first":
            if horizon is None or not 1 <= int(horizon) <= T:
                raise ValueError(f'blend_weights("first") needs 1 <= horizon <= seq_len={T}; got {horizon}')
            w = (t < int(horizon)).to(torch.float64)
        else:
            raise ValueError(f'blend kind must be "uniform", "exp" or "first"; got {kind!r}')
        return w.to(torch.float32).to(self.device)

    def _blend_windows(self, tokens, ntokens, starts, ends, num_frames, blend, fill, offset: int, want_counts: bool):
        """One launch of beast_reconstruct_windows_f32 (csrc/blend.hip).  The argument checks run before
        the device is asked for."""
        if self._basis.conditioned:
            raise NotImplementedError(
                "reconstruct_windows supports init_cond_order = end_cond_order = 0 only: the conditions are kept "
                "per batch from y0, y1 of materialised trajectories (uni_bspline.py:499-550), and a window "
                "table has none")
        src = tokens if tokens is not None else ntokens
        if not isinstance(src, torch.Tensor):
            src = torch.as_tensor(src)
        if src.dim() == 3:
            src = src.reshape(src.shape[0], -1)
        DN = self.num_basis * self.num_dof
        if src.dim() != 2 or src.shape[1] != DN:
            raise ValueError(f"tokens must be [W, num_basis*num_dof = {DN}] (or [W, num_basis, num_dof]); got "
                             f"{tuple(src.shape)}")
        if (tokens is not None) == src.dtype.is_floating_point or src.dtype is torch.bool:
            raise ValueError(f"{'tokens must be integers' if tokens is not None else 'params must be floating point'}; "
                             f"got {src.dtype}")
        if not isinstance(starts, torch.Tensor):
            starts = torch.as_tensor(starts)
        if not isinstance(ends, torch.Tensor):
            ends = torch.as_tensor(ends)
        if (starts.dim() != 1 or starts.shape != ends.shape or starts.dtype is not torch.int64
                or ends.dtype is not torch.int64):
            raise ValueError(f"starts / ends must be int64 [W] tables of one length; got {tuple(starts.shape)} "
                             f"{starts.dtype} and {tuple(ends.shape)} {ends.dtype}")
        W = starts.shape[0]
        if src.shape[0] != W:
            raise ValueError(f"{src.shape[0]} token rows for a table of {W} windows")
        R = int(num_frames)
        if R < 0:
            raise ValueError(f"num_frames must be >= 0; got {num_frames}")
        # host tables are checked here; a device table is not synchronised on (the kernel clamps it)
        if W and starts.device.type == "cpu" and ends.device.type == "cpu":
            if bool(((starts < 0) | (starts >= ends) | (ends > R)).any()):
                raise ValueError(f"window table out of range: need 0 <= start < end <= R={R} for every window")
            if bool((starts[1:] < starts[:-1]).any()):
                raise ValueError("window table is not sorted: starts must be non-decreasing (window_index builds "
                                 "such a table)")
        T = int(self.times.numel())
        if isinstance(blend, str):
            blend = self.blend_weights(blend)
        elif not isinstance(blend, torch.Tensor):
            blend = torch.as_tensor(blend, dtype=torch.float32)
        if blend.shape != (T,) or not blend.dtype.is_floating_point:
            raise ValueError(f"blend must be a floating-point [seq_len = {T}] tensor; got {tuple(blend.shape)} "
                             f"{blend.dtype}")
        if blend.device.type == "cpu" and not bool((torch.isfinite(blend) & (blend >= 0)).all()):
            raise ValueError("blend weights must be finite and >= 0")
        p = self._plan()
        dev = p.dev
        src = src.to(dev, dtype=torch.int64 if tokens is not None else torch.float32).contiguous()
        starts, ends = starts.to(dev).contiguous(), ends.to(dev).contiguous()
        blend = blend.to(dev, dtype=torch.float32).contiguous()
        D = self.num_dof
        frames = torch.empty((R, D), dtype=torch.float32, device=dev)
        coverage = torch.empty((R,), dtype=torch.int32, device=dev)
        weight = torch.empty((R,), dtype=torch.float32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev) if want_counts else None
        if R:
            # an empty tensor has no address to pass: an empty table's pointers are never read
            none = torch.zeros(2, dtype=torch.int64, device=dev).data_ptr() if W == 0 else None
            p_src = none or src.data_ptr()
            rc = p.rec_win(p_src if tokens is not None else None, None if tokens is not None else p_src, W, D,
                           self.joint_dof, self.num_basis, self.vocab_size, offset, p.p_wmn, p.p_wmx, p.p_phi, T,
                           none or starts.data_ptr(), none or ends.data_ptr(), R, blend.data_ptr(), float(fill),
                           p.p_dst, D, frames.data_ptr(), D, coverage.data_ptr(), weight.data_ptr(),
                           None if counts is None else counts.data_ptr(), _lib.raw_stream(p.idx))
            if rc:
                _lib.check(rc, "beast_reconstruct_windows_f32")
        info = {"coverage": coverage, "weight": weight}
        if want_counts:
            info["tile_counts"] = counts
        return frames, info

    @torch.no_grad()
    def reconstruct_windows(self, tokens, starts, ends, num_frames, *, blend="uniform", fill=float("nan"),
                            respect_llm_vocab_size=True, return_tile_counts=False):
        """The way back from ``encode_windows``: blend the tokens of a window table into the frames of a
        flat buffer, (frames fp32 [num_frames, num_dof], {"coverage": int32 [num_frames], "weight": fp32
        [num_frames]}), from one launch of ``beast_reconstruct_windows_f32`` on the current stream --
        no [W, seq_len, num_dof] intermediate and no atomics, so two runs agree bitwise.

        ``tokens`` int [W, num_basis*num_dof] as ``encode_windows`` returns them; ``starts`` / ``ends``
        int64 [W], the same table with the same meaning, and with non-decreasing starts
        (:meth:`window_index` builds such a table): window ``w`` owns the frames ``starts[w] + t`` for
        ``t < min(seq_len, ends[w] - starts[w])``; its edge-padding samples own nothing.  Frame ``r`` is
        ``sum_k blend[t_k] y_k / sum_k blend[t_k]`` over the windows that own it, in table order, with
        ``y_k`` bitwise ``reconstruct_traj``'s sample ``t_k = r - starts[w_k]`` of that window's tokens;
        samples whose blend weight is 0 are skipped.  ``coverage`` counts the
        contributors and ``weight`` is the denominator; frames nobody owns hold ``fill``.

        ``blend``: ``"uniform"``, ``"exp"`` (:meth:`blend_weights`' defaults) or a [seq_len] tensor
        (finite and >= 0: a host tensor is checked, a device tensor is not read back).  Host tables are
        checked for range and order (``ValueError``); device tables are never synchronised on: the
        kernel clamps them, so a bad one gives wrong numbers, never a fault.  ``return_tile_counts``
        adds ``"tile_counts"``: int32 [2], the chunks of candidate windows the kernel's row tiles
        walked / the tiles that walked more than one.  Tokenizers with init / end conditions raise
        ``NotImplementedError``."""
        return self._blend_windows(tokens, None, starts, ends, num_frames, blend, fill,
                                   self._offset(respect_llm_vocab_size), return_tile_counts)

    @torch.no_grad()
    def reconstruct_windows_continuous(self, params, starts, ends, num_frames, *, blend="uniform",
                                       fill=float("nan"), return_tile_counts=False):
        """``reconstruct_windows`` from normalised params in [-1, 1] ((t d) order, as
        ``encode_continuous_windows`` returns them and ``reconstruct_traj_continuous`` reads them)."""
        return self._blend_windows(None, params, starts, ends, num_frames, blend, fill, 0, return_tile_counts)

    # ===============================================
    #           - tokenizer LLM tokenization -
    # ===============================================

    def tokens_to_llm_tokens(self, tokens):
        tokens = tokens.to(self.device)
        if len(tokens.shape) == 3:
            tokens = tokens.reshape(tokens.shape[0], -1)
        if self.llm_vocab_size is None:
            raise ValueError("LLM vocab size is not set.")
        return tokens + self._llm_vocab_offset()

    def llm_tokens_to_mp_tokens(self, llm_tokens):
        if self.llm_vocab_size is None:
            raise ValueError("LLM vocab size is not set.")
        tokens = llm_tokens - self._llm_vocab_offset()
        if len(tokens.shape) == 2:
            tokens = tokens.reshape(tokens.shape[0], self.num_basis, self.num_dof)
        return tokens

    # ===============================================
    #            - tokenizer decoding -
    # ===============================================

    def reconstruct_from_llm_tokens(self, llm_tokens, times=None, **kwargs):
        # reference :479-481 (subtracts the offset here AND in decode: kept as-is)
        tokens = self.llm_tokens_to_mp_tokens(llm_tokens)
        return self.reconstruct_traj(tokens, times=times, **kwargs)

    def _token_rows(self, tokens, dev):
        if tokens.device != dev:
            tokens = tokens.to(dev)
        nd = tokens.dim()
        if nd == 3:
            tokens = tokens.reshape(tokens.shape[0], -1)
        elif nd != 2:
            raise ValueError(f"Unexpected token shape {tokens.shape}")
        if tokens.shape[1] != self.num_basis * self.num_dof:
            raise ValueError(f"Token dimension {tokens.shape[1]} does not match expected "
                             f"{self.num_basis * self.num_dof}.")
        if tokens.dtype is not torch.int64:
            tokens = tokens.to(torch.int64)
        return tokens if tokens.is_contiguous() else tokens.contiguous()

    def decode(self, tokens, *, respect_llm_vocab_size=True):
        """Dequantised params [B, num_dof*num_basis] in (d n) order (reference :483-496)."""
        p = self._plan()
        tokens = self._token_rows(tokens, p.dev)
        B = tokens.shape[0]
        params = torch.empty((B, self.num_dof * self.num_basis), dtype=torch.float32, device=p.dev)
        rc = p.rec(tokens.data_ptr(), B, self.num_dof, self.joint_dof, self.num_basis, self.vocab_size,
                   self._offset(respect_llm_vocab_size), p.p_wmn, p.p_wmx, None, 0, 0, None, self.num_dof, None,
                   0, None, params.data_ptr(), None, None, _lib.raw_stream(p.idx))
        if rc:
            _lib.check(rc, "beast_reconstruct_f32")
        return params

    def _basis_for(self, times, B: int, p: _Plan):
        """(basis tensor or None, basis ptr, batch stride, T_out) for reconstruct; the default grid is cached."""
        if times is None:
            return None, p.p_phi, 0, p.T
        N, dev = self.num_basis, p.dev
        t = times.to(dev, dtype=torch.float32)
        if t.dim() == 2 and t.shape[0] == B and (B == 1 or torch.equal(t, t[:1].expand_as(t))):
            t = t[0]
        if t.dim() == 1:
            Tn = t.numel()
            phi = torch.zeros((2, Tn, N), dtype=torch.float32, device=dev)
            phi[: self._basis.n_kinds] = self._basis.basis_at(t)
            return phi, phi.data_ptr(), 0, Tn
        if t.dim() != 2 or t.shape[0] != B:
            raise ValueError(f"times must be [T] or [B, T]; got {tuple(t.shape)} for B={B}")
        Tn = t.shape[1]
        phi_k = self._basis.basis_at(t)                       # [kinds, B, T, N]
        phi = torch.zeros((B, 2, Tn, N), dtype=torch.float32, device=dev)
        phi[:, : self._basis.n_kinds] = phi_k.permute(1, 0, 2, 3)
        return phi, phi.data_ptr(), 2 * Tn * N, Tn

    def _init_p_rows(self, init_p, B: int, p: _Plan):
        """init_p as the kernels read it (fp32 rows on the plan's device, unit column stride), or
        None where the reconstruction does not use it."""
        if init_p is None or not self.init_pos or self.joint_dof == 0:
            return None
        ip = torch.as_tensor(init_p).to(p.dev, dtype=torch.float32)
        if ip.dim() != 2 or ip.shape[0] != B:
            raise ValueError(f"init_p must be [B, num_dof]; got {tuple(ip.shape)}")
        return ip if ip.stride(1) == 1 else ip.contiguous()

    def _reconstruct(self, tokens, ntokens, times, init_p, respect_llm_vocab_size, p: _Plan, basis=None):
        src = tokens if tokens is not None else ntokens
        B = src.shape[0]
        D = self.num_dof
        phi, p_phi, basis_sb, Tn = basis or self._basis_for(times, B, p)
        pos = torch.empty((B, Tn, D), dtype=torch.float32, device=p.dev)
        ip, ip_sb, ip_src = self._init_p_rows(init_p, B, p), 0, None
        if ip is not None:
            ip_sb, ip_src = ip.stride(0), p.p_dst      # joint DoFs come first in the dof map
        offset = self._offset(respect_llm_vocab_size) if tokens is not None else 0
        rc = p.rec(None if tokens is None else tokens.data_ptr(), B, D, self.joint_dof, self.num_basis,
                   self.vocab_size, offset, p.p_wmn, p.p_wmx, p_phi, basis_sb, Tn, p.p_dst, D,
                   None if ip is None else ip.data_ptr(), ip_sb, ip_src, None, pos.data_ptr(),
                   None if ntokens is None else ntokens.data_ptr(), _lib.raw_stream(p.idx))
        if rc:
            _lib.check(rc, "beast_reconstruct_f32")
        if self._conditioned:
            pos = self._add_conditions(pos, times, B, p.dev)
        return pos

    def reconstruct_traj(self, tokens, times=None, **kwargs):
        """Positions [B, T, num_dof] from tokens (reference :498-536); kwargs: init_p [B, num_dof]."""
        p = self._plan()
        if times is None and not kwargs and p.fast_rec is not None:   # init_p=None takes the path below
            r = p.fast_rec(p.fast_addr, tokens, p.off)
            if r is not None:
                return r
        tokens = self._token_rows(tokens, p.dev)
        return self._reconstruct(tokens, None, times, kwargs.get("init_p"), True, p)

    @staticmethod
    def _wants_grad(params, init_p) -> bool:
        return torch.is_grad_enabled() and (params.requires_grad
                                            or (isinstance(init_p, torch.Tensor) and init_p.requires_grad))

    def reconstruct_traj_continuous(self, params, times=None, **kwargs):
        """Positions from normalised params in (t d) order (reference :538-582).

        Differentiable in ``params`` and a tensor ``init_p`` when one of them requires grad (one
        launch of ``beast_reconstruct_derivs_bwd_f32`` in the backward); any other
        call records no graph, as the reference's ``no_grad``."""
        p = self._plan()
        init_p = kwargs.get("init_p")
        grad = self._wants_grad(params, init_p)
        with torch.set_grad_enabled(grad):      # the move, reshape and cast carry the gradient back
            params = params.to(p.dev)
            if len(params.shape) == 3:
                params = params.reshape(params.shape[0], -1)
            if params.shape[-1] != self.num_basis * self.num_dof:
                raise ValueError(
                    f"Token dimension {params.shape[-1]} does not match expected {self.num_basis * self.num_dof}."
                )
            params = params.to(torch.float32).contiguous()
            if grad:
                ip = self._init_p_rows(init_p, params.shape[0], p)
                return _ReconstructContinuous.apply(params, ip, self, p, times, None)[0]
            return self._reconstruct(None, params, times, init_p, False, p)

    # ===============================================
    #     - decoding to velocity / acceleration -
    # ===============================================

    @staticmethod
    def _check_orders(orders) -> tuple:
        try:
            orders = tuple(orders)
        except TypeError:
            raise ValueError(f"orders must be a non-empty subset of (0, 1, 2); got {orders!r}") from None
        if (not orders or len(set(orders)) != len(orders)
                or any(isinstance(o, bool) or not isinstance(o, numbers.Integral) or o not in (0, 1, 2)
                       for o in orders)):
            raise ValueError(f"orders must be a non-empty subset of (0, 1, 2) without repeats; got {orders!r}")
        return tuple(int(o) for o in orders)

    def _deriv_basis_for(self, times, B: int, p: _Plan, orders: tuple):
        """(order slabs [3][2][T][N] or per row [B][3][2][T][N], batch stride, T_out) for
        beast_reconstruct_derivs_f32; the default grid's slabs are cached.  Only the requested
        orders' slabs are evaluated (the kernel reads no other)."""
        N, dev, kinds = self.num_basis, p.dev, self._basis.n_kinds
        if times is None:
            t = self.times.to(dev, dtype=torch.float32).reshape(-1)
            return self._basis.deriv_constants(t, self._times_version), 0, p.T
        t = times.to(dev, dtype=torch.float32)
        if t.dim() == 2 and t.shape[0] == B and (B == 1 or torch.equal(t, t[:1].expand_as(t))):
            t = t[0]
        if t.dim() == 1:
            Tn = t.numel()
            slabs = torch.zeros((3, 2, Tn, N), dtype=torch.float32, device=dev)
            for o in orders:
                slabs[o, :kinds] = self._basis.deriv_basis_at(t, o)
            return slabs, 0, Tn
        if t.dim() != 2 or t.shape[0] != B:
            raise ValueError(f"times must be [T] or [B, T]; got {tuple(t.shape)} for B={B}")
        Tn = t.shape[1]
        slabs = torch.zeros((B, 3, 2, Tn, N), dtype=torch.float32, device=dev)
        for o in orders:
            slabs[:, o, :kinds] = self._basis.deriv_basis_at(t, o).permute(1, 0, 2, 3)   # [kinds, B, T, N]
        return slabs, 3 * 2 * Tn * N, Tn

    def _reconstruct_derivs(self, tokens, ntokens, times, orders, init_p, respect_llm_vocab_size, p: _Plan,
                            basis=None):
        orders = self._check_orders(orders)
        src = tokens if tokens is not None else ntokens
        B, D = src.shape[0], self.num_dof
        slabs, basis_sb, Tn = basis or self._deriv_basis_for(times, B, p, orders)
        if Tn < 1:
            raise ValueError("times must hold at least one point")
        outs = [None, None, None]
        for o in orders:
            outs[o] = torch.empty((B, Tn, D), dtype=torch.float32, device=p.dev)
        if B == 0:
            return tuple(outs[o] for o in orders)
        ip, ip_sb, ip_src = self._init_p_rows(init_p, B, p), 0, None
        if ip is not None:
            ip_sb, ip_src = ip.stride(0), p.p_dst      # joint DoFs come first in the dof map
        offset = self._offset(respect_llm_vocab_size) if tokens is not None else 0
        _lib.run("beast_reconstruct_derivs_f32", _lib.ptr(tokens), B, D, self.joint_dof, self.num_basis,
                 self.vocab_size, offset, p.p_wmn, p.p_wmx, slabs.data_ptr(), basis_sb, Tn, p.p_dst, D,
                 _lib.ptr(ip), ip_sb, ip_src, *map(_lib.ptr, outs), _lib.ptr(ntokens), _lib.raw_stream(p.idx))
        if self._conditioned:
            for o in orders:
                outs[o] = self._add_conditions(outs[o], times, B, p.dev, order=o)
        return tuple(outs[o] for o in orders)

    def reconstruct_traj_derivs(self, tokens, times=None, orders=(0, 1, 2), *, init_p=None,
                                respect_llm_vocab_size=True):
        """Time derivatives of the decoded trajectory: a tuple of [B, T, num_dof] fp32 tensors, one
        per entry of ``orders`` (any non-empty subset of (0, 1, 2) without repeats: position,
        velocity, acceleration) in the order requested, from ONE launch of
        ``beast_reconstruct_derivs_f32`` -- the tokens are read and dequantised once.

        Order 1 is UniformBSpline.get_traj_vel (mp/uni_bspline.py:299-376); order 2 is the exact
        second time derivative, not get_traj_acc's value.  Gripper DoFs (degree 0)
        and any order above ``degree_p`` give zeros.  ``times`` is [T] or [B, T] as in
        ``reconstruct_traj``; outside [0, duration] the boundary's one-sided derivative is returned.
        With init / end conditions the last fit's conditions are used, as in ``reconstruct_traj``.

        No autograd graph is recorded: the outputs are written by the kernel into fresh tensors."""
        orders = self._check_orders(orders)
        p = self._plan()
        tokens = self._token_rows(tokens, p.dev)
        return self._reconstruct_derivs(tokens, None, times, orders, init_p, respect_llm_vocab_size, p)

    def reconstruct_traj_vel(self, tokens, times=None, **kwargs):
        """Velocities [B, T, num_dof]: ``reconstruct_traj_derivs(..., orders=(1,))[0]``."""
        return self.reconstruct_traj_derivs(tokens, times, (1,), **kwargs)[0]

    def reconstruct_traj_acc(self, tokens, times=None, **kwargs):
        """Accelerations [B, T, num_dof]: ``reconstruct_traj_derivs(..., orders=(2,))[0]``."""
        return self.reconstruct_traj_derivs(tokens, times, (2,), **kwargs)[0]

    def reconstruct_traj_continuous_derivs(self, params, times=None, orders=(0, 1, 2), **kwargs):
        """``reconstruct_traj_derivs`` from normalised params in (t d) order (the
        ``reconstruct_traj_continuous`` input); kwargs: init_p [B, num_dof].  Differentiable as
        ``reconstruct_traj_continuous`` is: every requested order feeds the one backward launch."""
        orders = self._check_orders(orders)
        p = self._plan()
        init_p = kwargs.get("init_p")
        grad = self._wants_grad(params, init_p)
        with torch.set_grad_enabled(grad):
            params = params.to(p.dev)
            if len(params.shape) == 3:
                params = params.reshape(params.shape[0], -1)
            if params.dim() != 2 or params.shape[-1] != self.num_basis * self.num_dof:
                raise ValueError(
                    f"Token dimension {params.shape[-1]} does not match expected {self.num_basis * self.num_dof}."
                )
            params = params.to(torch.float32).contiguous()
            if grad:
                ip = self._init_p_rows(init_p, params.shape[0], p)
                return _ReconstructContinuous.apply(params, ip, self, p, times, orders)
            return self._reconstruct_derivs(None, params, times, orders, init_p, False, p)

    # ===============================================
    #          - decoding from logits -
    # ===============================================

    def _check_logits(self, logits) -> None:
        """Shape and dtype of a logits argument; raised before the device is asked for."""
        K = self.num_basis * self.num_dof
        if not isinstance(logits, torch.Tensor) or not logits.dtype.is_floating_point:
            raise ValueError("logits must be a floating-point tensor")
        if logits.dtype not in _lib.LOGITS_DTYPES and logits.dtype is not torch.float64:
            raise ValueError(f"logits must be float32, float16, bfloat16 or float64; got {logits.dtype}")
        shape = tuple(logits.shape)
        if shape[1:-1] not in ((K,), (self.num_basis, self.num_dof)) or len(shape) < 3:
            raise ValueError(f"logits must be [B, {K}, V] or [B, {self.num_basis}, {self.num_dof}, V]; got {shape}")
        widths = {self.vocab_size} | ({self.llm_vocab_size} if self.llm_vocab_size is not None else set())
        if shape[-1] not in widths:
            raise ValueError(f"the last dimension of logits must be vocab_size {self.vocab_size}"
                             + (f" or llm_vocab_size {self.llm_vocab_size}" if self.llm_vocab_size is not None else "")
                             + f"; got {shape[-1]}")

    def _logits_rows(self, logits, dev: torch.device) -> torch.Tensor:
        """The action logits as the kernel reads them: [B, N*D, vocab_size] on ``dev``, fp32 / fp16 /
        bf16, unit last stride.  A full-vocabulary tensor gives the VIEW of its action slice
        [llm_vocab_size - vocab_size, llm_vocab_size): its strides go to the kernel, nothing is copied.
        Every step is a torch op, so under autograd the gradient finds its way back to the leaf."""
        if logits.device != dev:
            logits = logits.to(dev)
        if logits.dim() == 4:
            logits = logits.reshape(logits.shape[0], -1, logits.shape[-1])
        if logits.shape[-1] != self.vocab_size:
            logits = logits[..., self.llm_vocab_size - self.vocab_size:]
        if logits.dtype is torch.float64:
            logits = logits.to(torch.float32)
        return logits if logits.stride(2) == 1 else logits.contiguous()

    @staticmethod
    def _check_temperature(temperature) -> float:
        t = float(temperature)
        if not (t > 0.0 and t < float("inf")):
            raise ValueError(f"temperature must be finite and > 0; got {temperature!r}")
        return t

    @staticmethod
    def _check_truncation(top_k, top_p):
        """(top_k, top_p) as the kernels get them: 0 and 1.0 where off, top_p rounded to fp32."""
        if top_k is None:
            top_k = 0
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k < 2 ** 31:
            raise ValueError(f"top_k must be None or an integer >= 0; got {top_k!r}")
        try:
            p32 = 1.0 if top_p is None else struct.unpack("f", struct.pack("f", float(top_p)))[0]   # as the kernel gets it
        except (OverflowError, TypeError, ValueError):
            p32 = float("nan")
        if not 0.0 < p32 <= 1.0:
            raise ValueError(f"top_p must be None or lie in (0, 1]; got {top_p!r}")
        return top_k, p32

    def expected_params_from_logits(self, logits, *, temperature=1.0, return_tokens=False):
        """The expected normalised coefficients under ``softmax(logits / temperature)``: fp32
        [B, N*D] in (n d) order, the input of ``reconstruct_traj_continuous`` /
        ``reconstruct_traj_continuous_derivs``; with ``return_tokens`` also the greedy MP tokens
        (int64 [B, N*D], lowest bin on ties), from the same launch.

        ``logits`` is [B, N*D, V'] or [B, N, D, V'] with V' == vocab_size, or V' == llm_vocab_size
        when one is set (the action slice is then read in place).  fp32, fp16 and bf16 go to the
        kernel as they are.  Differentiable in ``logits`` (one launch of ``beast_logits_expect_bwd``,
        DESIGN.md §4); without ``requires_grad`` or under ``no_grad`` no graph is recorded."""
        self._check_logits(logits)
        temperature = self._check_temperature(temperature)
        p = self._plan()
        grad = torch.is_grad_enabled() and logits.requires_grad
        with torch.set_grad_enabled(grad):
            rows = self._logits_rows(logits, p.dev)
            if grad:
                return _ExpectedParams.apply(rows, temperature, bool(return_tokens))
            mean, tokens, _ = _logits_expect(rows, temperature, 0, True, bool(return_tokens), False)
            return (mean, tokens) if return_tokens else mean

    def reconstruct_traj_from_logits(self, logits, times=None, *, temperature=1.0, orders=None, init_p=None):
        """The trajectory of the expected coefficients: ``reconstruct_traj_continuous`` (``orders``
        None: positions [B, T, num_dof]) or ``reconstruct_traj_continuous_derivs`` (one tensor per
        requested order) applied to ``expected_params_from_logits``.  A trajectory-space loss reaches
        the logits through the two fused backward launches."""
        ntokens = self.expected_params_from_logits(logits, temperature=temperature)
        if orders is None:
            return self.reconstruct_traj_continuous(ntokens, times=times, init_p=init_p)
        return self.reconstruct_traj_continuous_derivs(ntokens, times=times, orders=orders, init_p=init_p)

    @torch.no_grad()
    def greedy_tokens_from_logits(self, logits, *, respect_llm_vocab_size=True):
        """Greedy tokens int64 [B, N*D]: the lowest bin that holds a row's maximum, over the action
        range only, plus the LLM offset exactly as ``encode`` adds it.  The same kernel with only its
        argmax output; never differentiable."""
        self._check_logits(logits)
        p = self._plan()
        rows = self._logits_rows(logits, p.dev)
        return _logits_expect(rows, 1.0, self._offset(respect_llm_vocab_size), False, True, False)[1]

    @torch.no_grad()
    def sample_tokens_from_logits(self, logits, *, temperature=1.0, top_k=None, top_p=None, num_samples=None,
                                  generator=None, uniforms=None, return_log_probs=False,
                                  respect_llm_vocab_size=True):
        """Tokens drawn from ``softmax(logits / temperature)`` over the action bins, from one fused
        launch that reads every row once for all draws: int64 [B, N*D], or
        [S, B, N*D] when ``num_samples`` = S (1 .. 64) is given, plus the LLM offset exactly as
        ``encode`` adds it, so they feed ``reconstruct_traj`` unchanged.  Never differentiable.

        ``logits`` is what ``greedy_tokens_from_logits`` takes.  ``top_k`` (None or 0: off) keeps the
        k largest logits and everything tied with the k-th; ``top_p`` (None or 1: off) then keeps the
        most probable bins whose renormalised mass reaches ``top_p``, a tie at the edge staying whole
        (DESIGN.md §8).  With ``return_log_probs`` the fp32 log-probabilities of the drawn tokens
        under the distribution actually drawn from (after temperature and truncation) come second,
        in the tokens' shape.

        The draws are inverse-CDF draws of uniforms in [0, 1): by default
        ``torch.rand((S, B, N*D), generator=generator)`` on the logits' device and the current stream;
        or the caller's ``uniforms`` of that shape ([B, N*D] or [B, N, D] too when ``num_samples`` is
        None), cast to fp32 -- the same uniforms give the same tokens, bit for bit."""
        self._check_logits(logits)
        temperature = self._check_temperature(temperature)
        K = self.num_basis * self.num_dof
        B = logits.shape[0]
        top_k, p32 = self._check_truncation(top_k, top_p)
        S = 1 if num_samples is None else num_samples
        if isinstance(S, bool) or not isinstance(S, int) or not 1 <= S <= SAMPLE_MAX_DRAWS:
            raise ValueError(f"num_samples must be None or an integer in [1, {SAMPLE_MAX_DRAWS}]; got {num_samples!r}")
        if uniforms is not None:
            if generator is not None:
                raise ValueError("give either generator or uniforms, not both")
            if not isinstance(uniforms, torch.Tensor) or not uniforms.dtype.is_floating_point:
                raise ValueError("uniforms must be a floating-point tensor")
            shapes = {(S, B, K), (S, B, self.num_basis, self.num_dof)}
            if num_samples is None:
                shapes |= {(B, K), (B, self.num_basis, self.num_dof)}
            if tuple(uniforms.shape) not in shapes:
                raise ValueError(f"uniforms must be [{S}, {B}, {K}]"
                                 + (f" or [{B}, {K}]" if num_samples is None else "")
                                 + f"; got {tuple(uniforms.shape)}")
        truncated = 0 < top_k < self.vocab_size or p32 < 1.0
        widest = 1024 if logits.dtype in (torch.float32, torch.float64) else 2048
        if truncated and self.vocab_size > widest:
            raise NotImplementedError(f"top_k / top_p are supported for vocab_size <= {widest} of {logits.dtype} "
                                      f"logits (vocab_size={self.vocab_size})")
        p = self._plan()
        rows = self._logits_rows(logits, p.dev)
        if uniforms is None:
            u = torch.rand((S, B, K), dtype=torch.float32, device=p.dev, generator=generator)
        else:
            u = uniforms.to(p.dev, dtype=torch.float32).reshape(S, B, K).contiguous()
        tokens, logprob, _ = _sample_rows(rows, u, temperature, top_k, p32, self._offset(respect_llm_vocab_size),
                                          bool(return_log_probs))
        if num_samples is None:
            tokens = tokens[0]
            logprob = logprob[0] if logprob is not None else None
        return (tokens, logprob) if return_log_probs else tokens

    def score_tokens_from_logits(self, logits, tokens=None, *, temperature=1.0, top_k=None, top_p=None,
                                 ref_logits=None, return_entropy=False, ignore_index=-100,
                                 respect_llm_vocab_size=True):
        """The fp32 log-probabilities of given ``tokens`` under exactly the distribution
        ``sample_tokens_from_logits`` draws from with the same ``temperature`` / ``top_k`` /
        ``top_p``, from one fused launch over the logits: scoring the tokens that call
        drew gives the bits of its ``return_log_probs``, so the importance ratio of an on-policy step
        is exactly 1.

        ``logits`` is what ``sample_tokens_from_logits`` takes.  ``tokens`` is integer, [B, N*D] or
        [B, N, D], or [S, B, N*D] or [S, B, N, D] with 1 <= S <= 64, carrying the LLM offset as
        ``encode`` / ``sample_tokens_from_logits`` give them; the result has their shape.  A token equal
        to ``ignore_index`` scores exactly 0, a token outside the kept set -inf (neither takes part in
        the backward), any other token outside the action range NaN.  ``tokens`` may be None when the
        entropy or the divergence is asked for.

        With ``return_entropy`` or ``ref_logits`` the result is the tuple ``(log_probs, entropy, kl)``,
        parts not asked for None: ``entropy`` [B, N*D] of the truncated, renormalised distribution and
        ``kl`` [B, N*D] its divergence from ``softmax(ref_logits / temperature)`` over all action bins.
        ``ref_logits`` has the logits' shape and dtype, is detached and never receives a gradient.

        Differentiable in ``logits`` for all three (one launch of ``beast_score_rows_bwd``, the kept
        set held constant, the gradient in the logits' own dtype); without ``requires_grad`` or under
        ``no_grad`` no graph is recorded."""
        self._check_logits(logits)
        temperature = self._check_temperature(temperature)
        N, D = self.num_basis, self.num_dof
        K = N * D
        B = logits.shape[0]
        top_k, p32 = self._check_truncation(top_k, top_p)
        S = None
        if tokens is not None:
            if not isinstance(tokens, torch.Tensor) or tokens.dtype.is_floating_point or tokens.is_complex() \
                    or tokens.dtype is torch.bool:
                raise ValueError("tokens must be an integer tensor")
            shape = tuple(tokens.shape)
            if shape in ((B, K), (B, N, D)):
                S = 0                                          # no leading axis
            elif shape[1:] in ((B, K), (B, N, D)) and 1 <= shape[0] <= SAMPLE_MAX_DRAWS:
                S = shape[0]
            else:
                raise ValueError(f"tokens must be [{B}, {K}], [{B}, {N}, {D}] or the same behind a leading axis of "
                                 f"1 .. {SAMPLE_MAX_DRAWS} draws; got {shape}")
        elif not return_entropy and ref_logits is None:
            raise ValueError("tokens may be None only when return_entropy or ref_logits is given")
        if ref_logits is not None:
            if not isinstance(ref_logits, torch.Tensor) or tuple(ref_logits.shape) != tuple(logits.shape):
                raise ValueError(f"ref_logits must have the logits' shape {tuple(logits.shape)}")
            if ref_logits.dtype != logits.dtype:
                raise ValueError(f"ref_logits must have the logits' dtype {logits.dtype}; got {ref_logits.dtype}")
        ignore_index = int(ignore_index)
        truncated = 0 < top_k < self.vocab_size or p32 < 1.0
        widest = 1024 if logits.dtype in (torch.float32, torch.float64) else 2048
        if truncated and self.vocab_size > widest:
            raise NotImplementedError(f"top_k / top_p are supported for vocab_size <= {widest} of {logits.dtype} "
                                      f"logits (vocab_size={self.vocab_size})")
        p = self._plan()
        grad = torch.is_grad_enabled() and logits.requires_grad
        consts = (temperature, top_k, p32, self._offset(respect_llm_vocab_size), ignore_index)
        with torch.no_grad():
            tok = None
            if tokens is not None:
                tok = tokens.detach().to(p.dev, dtype=torch.int64).reshape(max(S, 1), B, K).contiguous()
            ref = None if ref_logits is None else self._logits_rows(ref_logits.detach(), p.dev)
        with torch.set_grad_enabled(grad):
            rows = self._logits_rows(logits, p.dev)
            if grad:
                logprob, entropy, kl = _ScoreTokens.apply(rows, ref, tok, consts, bool(return_entropy))
                logprob = logprob if tok is not None else None
                entropy = entropy if return_entropy else None
                kl = kl if ref is not None else None
            else:
                logprob, entropy, kl, _ = _score_rows(rows, ref, tok, *consts, bool(return_entropy), False)
            if logprob is not None:
                logprob = logprob.reshape(tokens.shape)
        return (logprob, entropy, kl) if (return_entropy or ref_logits is not None) else logprob

    # ===============================================
    #          - training from logits -
    # ===============================================

    def _check_xent_target(self, target, batch: int) -> None:
        """Shape and dtype of a cross-entropy target; raised before the device is asked for."""
        K = self.num_basis * self.num_dof
        if not isinstance(target, torch.Tensor) or target.dtype is torch.bool or target.is_complex():
            raise ValueError("target must be an integer tensor of tokens or a floating-point tensor of "
                             "normalised coefficients")
        if tuple(target.shape) not in ((batch, K), (batch, self.num_basis, self.num_dof)):
            raise ValueError(f"target must be [{batch}, {K}] or [{batch}, {self.num_basis}, {self.num_dof}]; "
                             f"got {tuple(target.shape)}")

    def cross_entropy_from_logits(self, logits, target, *, label_smoothing=0.0, ignore_index=-100,
                                  reduction="mean", return_tokens=False, respect_llm_vocab_size=True):
        """The token loss of a discrete head, from one fused launch over the logits.

        ``logits`` is what ``expected_params_from_logits`` takes.  The softmax runs over the
        ``vocab_size`` action bins only: of a full-vocabulary tensor only the action slice is read,
        and only it receives a gradient.  ``target`` is [B, N*D] or [B, N, D] and selects the loss:

        * integer tokens, as ``encode`` returns them (the LLM offset is removed in the kernel
          according to ``respect_llm_vocab_size``): the usual cross-entropy.  Rows whose token equals
          ``ignore_index`` are ignored; any other token outside the action range gives NaN.
        * floating-point normalised coefficients in [-1, 1] in the same (n d) order, as
          ``encode_continuous`` returns them and ``reconstruct_traj_continuous`` takes them: the
          two-hot target on the two bins around the coefficient, whose expectation is the coefficient
          itself, so the optimum agrees with ``expected_params_from_logits``.  NaN coefficients are
          ignored.

        ``label_smoothing`` in [0, 1) mixes the target with the uniform distribution.  ``reduction``
        "none" gives fp32 [B, N*D]; "sum" and "mean" reduce it with torch ops, "mean" over the rows
        that are not ignored (NaN when there are none).  With ``return_tokens`` the greedy MP tokens
        of the same launch come second.  Differentiable in ``logits`` (one launch of
        ``beast_xent_rows_bwd``); without ``requires_grad`` or under ``no_grad`` no graph is recorded."""
        self._check_logits(logits)
        self._check_xent_target(target, logits.shape[0])
        try:
            smoothing = struct.unpack("f", struct.pack("f", float(label_smoothing)))[0]   # as the kernel gets it
        except (OverflowError, TypeError, ValueError):
            smoothing = float("nan")
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1); got {label_smoothing!r}")
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(f"reduction must be 'none', 'sum' or 'mean'; got {reduction!r}")
        ignore_index = int(ignore_index)
        p = self._plan()
        grad = torch.is_grad_enabled() and logits.requires_grad
        off = self._offset(respect_llm_vocab_size)
        with torch.no_grad():
            tgt = target.detach().to(p.dev).reshape(target.shape[0], self.num_basis * self.num_dof)
            tgt = tgt.to(torch.float32 if tgt.dtype.is_floating_point else torch.int64).contiguous()
        with torch.set_grad_enabled(grad):
            rows = self._logits_rows(logits, p.dev)
            if grad:
                out = _CrossEntropy.apply(rows, tgt, off, ignore_index, smoothing, bool(return_tokens))
                loss, tokens = out if return_tokens else (out, None)
            else:
                loss, tokens, _ = _xent_rows(rows, tgt, off, ignore_index, smoothing, True, bool(return_tokens), False)
            if reduction != "none":
                total = loss.sum()
                if reduction == "mean":
                    kept = ~torch.isnan(tgt) if tgt.dtype.is_floating_point else tgt != ignore_index
                    total = total / kept.sum()
                loss = total
        return (loss, tokens) if return_tokens else loss

    # ===============================================
    #           - tokenizer evaluation -
    # ===============================================

    def _scatter_cols(self, x: torch.Tensor) -> torch.Tensor:
        """[B, D] in DoF order (joint ++ gripper) -> [B, num_dof] in output-column order."""
        order = self.joint_indices + self.gripper_indices
        if order == list(range(len(order))):
            return x
        out = torch.empty_like(x)
        out[:, torch.as_tensor(order, device=x.device)] = x
        return out

    @torch.no_grad()
    def reconstruction_stats(self, trajs, *, return_tokens=False, respect_llm_vocab_size=True):
        """Per-trajectory, per-column error of encode -> reconstruct as a ``ReconstructionStats``,
        from ONE launch of ``beast_roundtrip_stats_f32``: the trajectory is read once and neither
        tokens, params nor positions travel through memory (the tokens only with
        ``return_tokens``).  ``mse`` / ``mean_err`` / ``max_abs`` compare the input with exactly what
        ``reconstruct_traj(encode(trajs)[0])`` returns; ``mse_fit`` is the same for the unquantised
        spline fit, so ``mse - mse_fit`` is what clamping and quantisation add; ``clip_low`` /
        ``clip_high`` count the trajectories whose params the bounds clamp.  ``.l2`` / ``.l1`` are
        ``compute_reconstruction_error``'s two batch means.

        ``trajs`` as for ``encode``: [B, T, >= num_dof] (or one [T, D] trajectory), any strides; other
        dtypes are cast to fp32.  Tokenizers with init / end conditions take the composed path
        (``encode`` + ``reconstruct_traj`` + torch reductions; ``encode`` stores the conditions as
        usual) and return ``mse_fit = None``."""
        p = self._plan()
        trajs = torch.as_tensor(trajs)
        if trajs.device != p.dev or trajs.dtype is not torch.float32:
            trajs = trajs.to(p.dev, dtype=torch.float32)
        if trajs.dim() == 2:
            trajs = trajs.unsqueeze(0)
        shape = trajs.shape
        if len(shape) != 3 or shape[1] != p.T:
            raise AssertionError(f"trajectory shape {tuple(shape)} does not match [B, {p.T}, num_dof] time grid")
        B, T, Din = shape
        if Din < p.min_din:
            raise IndexError(f"index {p.min_din - 1} is out of bounds for dimension 2 with size {Din}")
        D, N = self.num_dof, self.num_basis
        offset = p.off if respect_llm_vocab_size else 0
        if self._conditioned:
            params, tokens = self._fit(trajs, offset, p)
            pos = self._reconstruct(tokens, None, None, None, respect_llm_vocab_size, p)
            err = trajs[..., :D] - pos
            wmn, wmx = self._bounds(p.dev)
            return ReconstructionStats((err * err).mean(dim=1), err.mean(dim=1), err.abs().amax(dim=1), None,
                                       (params < wmn).sum(dim=0).reshape(D, N),
                                       (params > wmx).sum(dim=0).reshape(D, N), tokens if return_tokens else None)
        st = trajs.stride()
        tokens = torch.empty((B, N * D), dtype=torch.int64, device=p.dev) if return_tokens else None
        stats = torch.empty((B, D, 4), dtype=torch.float32, device=p.dev)
        clip = torch.zeros((2, D * N), dtype=torch.int32, device=p.dev)   # the kernel's uint32 counters
        _lib.run("beast_roundtrip_stats_f32", trajs.data_ptr(), B, T, st[0], st[1], st[2], Din, D, self.joint_dof,
                 p.p_src, p.p_proj, p.p_phi, N, p.p_wmn, p.p_wmx, self.vocab_size, offset, _lib.ptr(tokens),
                 stats.data_ptr(), clip.data_ptr(), _lib.raw_stream(p.idx))
        inv_t = 1.0 / T
        clip = clip.to(torch.int64).reshape(2, D, N)
        return ReconstructionStats(self._scatter_cols(stats[..., 1] * inv_t), self._scatter_cols(stats[..., 0] * inv_t),
                                   self._scatter_cols(stats[..., 2]), self._scatter_cols(stats[..., 3] * inv_t),
                                   clip[0], clip[1], tokens)

    @torch.no_grad()
    def evaluate_reconstruction(self, dataloader, max_samples=None):
        """``reconstruction_stats`` over a dataloader, accumulated on the device in float64 / int64
        without a host synchronisation per batch.  Batches as for ``fit_parameters`` (a tensor, or
        a dict with an ``"actions"`` entry; the last batch may be smaller); ``max_samples`` counts
        batches, as it does there.  Returns a dict: ``mse``, ``mean_err``, ``max_abs``, ``mse_fit``
        (float64 [num_dof], per output column: the means / the maximum over every trajectory seen;
        ``mse_fit`` is None with init / end conditions), ``clip_low_rate``, ``clip_high_rate``
        (float64 [num_dof, num_basis]: the share of trajectories whose param the bound clamps),
        ``clip_low``, ``clip_high`` (the int64 counts) and ``num_samples`` (trajectories)."""
        limit = max_samples if max_samples is not None else float("inf")
        acc = None
        count = batches = 0
        for batch in dataloader:
            if isinstance(batch, torch.Tensor):
                actions = batch
            else:
                if "actions" not in batch:
                    raise KeyError("Expected batch to contain an 'actions' entry.")
                actions = batch["actions"]
            r = self.reconstruction_stats(actions[..., : self.num_dof])
            if r.mse.shape[0]:
                cur = [r.mse.double().sum(dim=0), r.mean_err.double().sum(dim=0), r.max_abs.double().amax(dim=0),
                       None if r.mse_fit is None else r.mse_fit.double().sum(dim=0), r.clip_low, r.clip_high]
                if acc is None:
                    acc = cur
                else:
                    acc = [None if a is None else (torch.maximum(a, c) if i == 2 else a + c)
                           for i, (a, c) in enumerate(zip(acc, cur))]
                count += r.mse.shape[0]
            batches += 1
            if batches >= limit:
                break
        if acc is None:
            raise RuntimeError("No trajectories were gathered from the dataloader.")
        return {"mse": acc[0] / count, "mean_err": acc[1] / count, "max_abs": acc[2],
                "mse_fit": None if acc[3] is None else acc[3] / count,
                "clip_low_rate": acc[4].double() / count, "clip_high_rate": acc[5].double() / count,
                "clip_low": acc[4], "clip_high": acc[5], "num_samples": count}

    def compute_reconstruction_error(self, raw_traj, return_tokens=False):
        """(mean squared error, mean signed error) of encode -> reconstruct (reference :589-597)."""
        dev = self._dev()
        raw_traj = raw_traj.to(dev, dtype=torch.float32)
        if len(raw_traj.shape) == 2:
            raw_traj = raw_traj.unsqueeze(0)
        tokens, _ = self.encode(raw_traj)
        reconstruct_trajs = self.reconstruct_traj(tokens)
        error_l2 = torch.mean((raw_traj - reconstruct_trajs) ** 2)
        error_l1 = torch.mean(raw_traj - reconstruct_trajs)
        if return_tokens:
            return error_l2, error_l1, tokens
        return error_l2, error_l1
