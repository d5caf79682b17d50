"""Autograd wrappers of the non-chain kernels: layout changes, mean aggregation over the
points of a task, and the Gaussian head.  Every function launches HIP kernels through the
C ABI (``_lib``); none has a CPU path."""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from . import chain as CH
from .chain import pad32, pt_empty, pt_shape, tiles_of


# ---- layout ---------------------------------------------------------------------------
def _pack(rows: torch.Tensor) -> torch.Tensor:
    n_tasks, pts, F = rows.shape
    out = pt_empty(n_tasks, pts, F, rows.device)
    L.check(L.load().npf_pack_pt(L.ptr(rows.contiguous()), n_tasks, pts, F, L.ptr(out), L.stream_ptr()), "npf_pack_pt")
    return out


def _unpack(pt: torch.Tensor, pts: int, F: int) -> torch.Tensor:
    n_tasks = pt.shape[0]
    out = torch.empty((n_tasks, pts, F), dtype=torch.float32, device=pt.device)
    L.check(L.load().npf_unpack_pt(L.ptr(pt.contiguous()), n_tasks, pts, F, L.ptr(out), L.stream_ptr()), "npf_unpack_pt")
    return out


class _PackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows):
        ctx.pts, ctx.F = rows.shape[1], rows.shape[2]
        return _pack(rows)

    @staticmethod
    def backward(ctx, g):
        return _unpack(g.contiguous(), ctx.pts, ctx.F)


class _UnpackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pt, pts, F):
        return _unpack(pt, pts, F)

    @staticmethod
    def backward(ctx, g):
        return _pack(g.contiguous()), None, None


def pack_pt(rows: torch.Tensor) -> torch.Tensor:
    """row-major [n_tasks, pts, F] -> PT32 (padding points / features are zero)."""
    return _PackFn.apply(rows)


def unpack_pt(pt: torch.Tensor, pts: int, F: int) -> torch.Tensor:
    """PT32 -> row-major [n_tasks, pts, F]."""
    return _UnpackFn.apply(pt, pts, F)


# ---- mean over the points of a task ---------------------------------------------------
def sum_points_pt(pt: torch.Tensor, pts: int, F: int) -> torch.Tensor:
    """[n_tasks, pad32(F)] sum over the valid points (no autograd)."""
    n_tasks = pt.shape[0]
    Fp = pad32(F)
    out = torch.empty((n_tasks, Fp), dtype=torch.float32, device=pt.device)
    L.check(L.load().npf_mean_agg_fwd(L.ptr(pt), n_tasks, pts, Fp, L.ptr(out), L.stream_ptr()), "npf_mean_agg_fwd")
    return out * float(pts)


class _MeanFn(torch.autograd.Function):
    """Mean over all points of every task (``n_valid`` None: ``npf_mean_agg_fwd`` / ``_bwd``) or over the first ``n_valid[task]`` of
    them (a device int32 tensor: ``npf_masked_mean_fwd`` / ``_bwd``)."""

    @staticmethod
    def forward(ctx, pt, n_valid, n_tasks, pts, F):
        Fp = pad32(F)
        ctx.geo = (n_tasks, pts, Fp)
        if n_valid is not None:
            ctx.save_for_backward(n_valid)
        out = torch.empty((n_tasks, Fp), dtype=torch.float32, device=pt.device)
        name, counts = ("npf_mean_agg_fwd", ()) if n_valid is None else ("npf_masked_mean_fwd", (_iptr(n_valid),))
        L.check(getattr(L.load(), name)(L.ptr(pt.contiguous()), *counts, n_tasks, pts, Fp, L.ptr(out), L.stream_ptr()), name)
        return out

    @staticmethod
    def backward(ctx, g):
        n_tasks, pts, Fp = ctx.geo
        d = pt_empty(n_tasks, pts, Fp, g.device)
        name, counts = ("npf_masked_mean_bwd", (_iptr(ctx.saved_tensors[0]),)) if ctx.saved_tensors else ("npf_mean_agg_bwd", ())
        L.check(getattr(L.load(), name)(L.ptr(g.contiguous()), *counts, n_tasks, pts, Fp, L.ptr(d), 0, L.stream_ptr()), name)
        return d, None, None, None, None


def mean_agg(pt: torch.Tensor, pts: int, F: int) -> torch.Tensor:
    """torch.mean(R, dim=1) of a PT32 tensor -> row-major [n_tasks, pad32(F)]
    (npf/neuralproc/np.py:95, attnnp.py:181)."""
    return _MeanFn.apply(pt, None, pt.shape[0], pts, F)


# ---- Gaussian head --------------------------------------------------------------------
class _GaussHeadFn(torch.autograd.Function):
    """The head of every row over all its points (``n_valid`` None: ``npf_gauss_head_fwd`` / ``_bwd``) or over padded targets, row
    ``r`` owning its first ``n_valid[r % n_tasks]`` points (a device int32 tensor: ``npf_masked_gauss_head_fwd`` / ``_bwd``).  Beyond
    the count: loc = 0, scale = 1, nothing in ``sum_log_prob``, zero rows in the gradient."""

    @staticmethod
    def forward(ctx, suff, Y, n_valid, dy, homosk, want_dist):
        n_rows, pts, two_dy = suff.shape
        n_tasks = 1 if n_valid is None else n_valid.shape[0]
        assert two_dy == 2 * dy and n_rows % n_tasks == 0
        suff = suff.contiguous()
        loc = scale = None
        if want_dist:
            loc = torch.empty((n_rows, pts, dy), dtype=torch.float32, device=suff.device)
            scale = torch.empty_like(loc)
        slp = None
        n_y = 0
        if Y is not None:
            Y = Y.contiguous()
            n_y = Y.shape[0]
            assert Y.shape[1:] == (pts, dy) and n_rows % n_y == 0 and n_y % n_tasks == 0
            slp = torch.empty((n_rows,), dtype=torch.float32, device=suff.device)
        elif not want_dist:
            raise ValueError("a loss-only head launch needs the targets")
        name, counts = ("npf_gauss_head_fwd", ()) if n_valid is None else ("npf_masked_gauss_head_fwd", (_iptr(n_valid), n_tasks))
        L.check(getattr(L.load(), name)(L.ptr(suff), *counts, n_rows, pts, dy, int(homosk), L.ptr(Y), n_y, L.ptr(loc), L.ptr(scale),
                                        L.ptr(slp), L.stream_ptr()), name)
        ctx.save_for_backward(suff, loc, scale, Y, *(() if n_valid is None else (n_valid,)))
        ctx.cfg = (dy, homosk)
        empty = suff.new_zeros((0,))
        outs = [loc if want_dist else empty, scale if want_dist else empty, slp if slp is not None else suff.new_zeros((n_rows,))]
        nd = ([] if want_dist else [outs[0], outs[1]]) + ([] if slp is not None else [outs[2]])
        if nd:
            ctx.mark_non_differentiable(*nd)
        return tuple(outs)

    @staticmethod
    def backward(ctx, d_loc, d_scale, d_slp):
        suff, loc, scale, Y, *n_valid = ctx.saved_tensors
        dy, homosk = ctx.cfg
        n_rows, pts, _ = suff.shape
        d_suff = torch.empty_like(suff)  # (written whole: zeros beyond the count)
        c = lambda t: t.contiguous() if t is not None else None  # noqa: E731
        if loc is None:
            d_loc = d_scale = None
        name, counts = ("npf_masked_gauss_head_bwd", (_iptr(n_valid[0]), n_valid[0].shape[0])) if n_valid else ("npf_gauss_head_bwd", ())
        L.check(getattr(L.load(), name)(L.ptr(suff), L.ptr(loc), L.ptr(scale), *counts, n_rows, pts, dy, int(homosk), L.ptr(Y),
                                        Y.shape[0] if Y is not None else 0, L.ptr(c(d_loc)), L.ptr(c(d_scale)),
                                        L.ptr(c(d_slp)) if Y is not None else None, L.ptr(d_suff), L.stream_ptr()), name)
        return d_suff, None, None, None, None, None


def gauss_head(suff: torch.Tensor, Y: Optional[torch.Tensor], dy: int, homoskedastic: bool, want_dist: bool = True,
               n_valid: Optional[torch.Tensor] = None):
    """(loc, scale, sum_log_prob) from the raw decoder output ``suff`` [rows, pts, 2*dy]
    (npf/neuralproc/base.py:350-365; losses.py:18-24).  ``sum_log_prob`` [rows] is the
    log-likelihood of ``Y`` [rows or B, pts, dy] summed over targets and y-dims.  ``want_dist=False``: a
    loss-only launch -- loc and scale come back empty and nothing of size [rows, pts, dy] is written.
    ``n_valid``: device integer tensor [n_tasks] (``rows`` a multiple of it, row ``r`` is task ``r % n_tasks``), the number of real
    points of every task of a padded batch: sums and the homoskedastic pooling cover the rows below the count only, beyond it
    loc = 0 and scale = 1, ``Y`` there is never read and the gradient rows are zeros (``npf_masked_gauss_head_fwd`` / ``_bwd``)."""
    if n_valid is not None:
        n_tasks = n_valid.shape[0] if isinstance(n_valid, torch.Tensor) and n_valid.dim() == 1 else suff.shape[0]
        if suff.shape[0] % max(n_tasks, 1) != 0 or n_tasks == 0:
            raise ValueError(f"n_valid has {n_tasks} counts, the head {suff.shape[0]} rows (not a multiple)")
        n_valid = counts_i32(n_valid, n_tasks)
    return _GaussHeadFn.apply(suff, Y, n_valid, dy, homoskedastic, want_dist)


# ---- predictive summary over the latent samples -------------------------------------------
MIXTURE_MAX_NZ = 128  # latent samples npf_mixture_summary covers
_Z_P_CACHE = {}       # (probs, device) -> (z_p, probs) device float32 tensors


def check_probs(probs) -> tuple:
    """``probs`` as a tuple of host floats strictly inside (0, 1); anything else -- a tensor, a scalar, 0, 1 -- is a ValueError."""
    if isinstance(probs, torch.Tensor) or not isinstance(probs, (tuple, list)):
        raise ValueError(f"probs must be a host sequence (tuple / list) of probabilities, got {type(probs).__name__}")
    out = []
    for p in probs:
        if isinstance(p, torch.Tensor) or isinstance(p, bool) or not isinstance(p, (int, float)):
            raise ValueError(f"probs must hold host floats, got {type(p).__name__}")
        if not (0.0 < float(p) < 1.0):
            raise ValueError(f"probs must lie strictly inside (0, 1), got {p}")
        out.append(float(p))
    return tuple(out)


def normal_quantiles(probs) -> tuple:
    """The standard-normal quantiles of ``probs`` as host floats, computed in float64 (``torch.special.ndtri`` on the CPU)."""
    probs = check_probs(probs)
    if not probs:
        return ()
    return tuple(torch.special.ndtri(torch.tensor(probs, dtype=torch.float64)).tolist())


def _z_p_device(probs: tuple, device: torch.device):
    """(z_p, probs) as device float32 tensors, uploaded once per (probs, device): a captured replay uploads nothing."""
    key = (probs, device.type, device.index if device.index is not None else torch.cuda.current_device())
    hit = _Z_P_CACHE.get(key)
    if hit is None:
        hit = (torch.tensor(normal_quantiles(probs), dtype=torch.float64).to(torch.float32).to(device),
               torch.tensor(probs, dtype=torch.float64).to(torch.float32).to(device))
        _Z_P_CACHE[key] = hit
    return hit


def mixture_summary(suff: torch.Tensor, n_z: int, dy: int, homoskedastic: bool, probs=(), n_valid: Optional[torch.Tensor] = None):
    """(mean, std, quantiles) of the equal-weight mixture over the latent samples of the Gaussians the head makes of the raw decoder
    output ``suff`` [n_z * B, pts, 2 * dy] (row ``k * B + b``): ``mean`` / ``std`` [B, pts, dy], ``quantiles`` [len(probs), B, pts, dy].
    One ``npf_mixture_summary`` launch, inference only (no autograd); nothing of size [n_z, B, pts, dy] is written.  ``probs``: a host
    sequence of probabilities strictly inside (0, 1).  ``n_valid``: device integer tensor [B], the real points of every task of a
    padded batch (rows beyond: mean 0, std 1, the standard-normal quantiles)."""
    probs = check_probs(probs)
    if not suff.is_cuda or suff.dtype != torch.float32:
        raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    n_rows, pts, two_dy = suff.shape
    if two_dy != 2 * dy or n_z < 1 or n_rows % n_z != 0:
        raise ValueError(f"suff of shape {tuple(suff.shape)} does not hold n_z={n_z} samples of a {dy}-dimensional head")
    if n_z > MIXTURE_MAX_NZ:
        raise NotImplementedError(f"mixture_summary covers up to {MIXTURE_MAX_NZ} latent samples (got {n_z})")
    B = n_rows // n_z
    suff = suff.detach().contiguous()
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    mean = torch.empty((B, pts, dy), dtype=torch.float32, device=suff.device)
    std = torch.empty_like(mean)
    quant = torch.empty((len(probs), B, pts, dy), dtype=torch.float32, device=suff.device)
    z_p, p_dev = _z_p_device(probs, suff.device) if probs else (None, None)
    L.check(L.load().npf_mixture_summary(L.ptr(suff), _iptr(nv) if nv is not None else None, n_z, B, pts, dy, int(homoskedastic),
                                         L.ptr(z_p), len(probs), L.ptr(p_dev), L.ptr(mean), L.ptr(std),
                                         L.ptr(quant) if probs else None, L.stream_ptr()), "npf_mixture_summary")
    return mean, std, quant


SCORE_NAMES = ("log_density", "pit", "crps")


def check_want(want) -> tuple:
    """``want`` as a tuple of names out of ``SCORE_NAMES``, at least one; anything else is a ValueError."""
    if isinstance(want, str) or not isinstance(want, (tuple, list)):
        raise ValueError(f"want must be a tuple / list of names out of {SCORE_NAMES}, got {want!r}")
    for w in want:
        if w not in SCORE_NAMES:
            raise ValueError(f"want: unknown score {w!r} (known: {SCORE_NAMES})")
    if not want:
        raise ValueError(f"want must name at least one of {SCORE_NAMES}")
    return tuple(want)


def mixture_score(suff: torch.Tensor, Y: torch.Tensor, n_z: int, dy: int, homoskedastic: bool, n_valid: Optional[torch.Tensor] = None,
                  want=SCORE_NAMES):
    """(log_density, pit, crps) at the observations ``Y`` [B, pts, dy] of the equal-weight mixture over the latent samples of the
    Gaussians the head makes of the raw decoder output ``suff`` [n_z * B, pts, 2 * dy] (row ``k * B + b``): [B, pts, dy] each,
    marginal per output dimension; the entries ``want`` does not name are ``None`` and cost nothing.  One ``npf_mixture_score``
    launch, inference only (no autograd), no host sync; nothing of size [n_z, B, pts, dy] is written.  ``log_density`` is the log of
    the mixture density, ``pit`` its CDF at ``Y`` (the probability integral transform) and ``crps`` the continuous ranked probability
    score in closed form (``include/npf_hip.h`` has the formulae).  ``n_valid``: device integer tensor [B], the real points of every
    task of a padded batch; rows beyond hold ``log_density = 0``, ``crps = 0`` (a sum over the points needs no mask) and
    ``pit = 0.5``: a PIT histogram must be masked by the counts."""
    want = check_want(want)
    if not suff.is_cuda or suff.dtype != torch.float32 or not Y.is_cuda or Y.dtype != torch.float32:
        raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    n_rows, pts, two_dy = suff.shape
    if two_dy != 2 * dy or n_z < 1 or n_rows % n_z != 0:
        raise ValueError(f"suff of shape {tuple(suff.shape)} does not hold n_z={n_z} samples of a {dy}-dimensional head")
    if n_z > MIXTURE_MAX_NZ:
        raise NotImplementedError(f"mixture_score covers up to {MIXTURE_MAX_NZ} latent samples (got {n_z})")
    B = n_rows // n_z
    if tuple(Y.shape) != (B, pts, dy):
        raise ValueError(f"Y must have shape [B={B}, pts={pts}, dy={dy}], got {tuple(Y.shape)}")
    suff, Y = suff.detach().contiguous(), Y.detach().contiguous()
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    out = [torch.empty((B, pts, dy), dtype=torch.float32, device=suff.device) if name in want else None for name in SCORE_NAMES]
    L.check(L.load().npf_mixture_score(L.ptr(suff), L.ptr(Y), _iptr(nv) if nv is not None else None, n_z, B, pts, dy,
                                       int(homoskedastic), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.stream_ptr()),
            "npf_mixture_score")
    return tuple(out)


# ---- waveform match over a time-shift grid (csrc/waveform_kernels.hip) ----------------------
MATCH_NAMES = ("hh", "gg", "overlap", "match", "mismatch", "tau_index", "phase")
MATCH_JC = 16            # time shifts per workgroup of the correlation launch (NPF_WAVEFORM_JC)
MATCH_MAX_TAU = 65536    # longest time-shift grid
_MATCH_WS = {}           # device index -> [float64 workspaces], the last one in use; grown ones are kept (a captured graph holds them)


class WaveformMatch(NamedTuple):
    """What :func:`waveform_match` returns; the entries that were not asked for are ``None``."""
    hh: Optional[torch.Tensor]         # [R] sum_t w A^2
    gg: Optional[torch.Tensor]         # [B] sum_t w A'^2
    overlap: Optional[torch.Tensor]    # [R]
    match: Optional[torch.Tensor]      # [R]
    mismatch: Optional[torch.Tensor]   # [R]
    tau_index: Optional[torch.Tensor]  # [R] int32
    phase: Optional[torch.Tensor]      # [R]
    corr: Optional[torch.Tensor]       # [R, max(n_tau, 1), 2]


def check_match_want(want) -> tuple:
    """``want`` as a tuple of names out of ``MATCH_NAMES`` (may be empty: ``corr`` alone); anything else is a ValueError."""
    if isinstance(want, str) or not isinstance(want, (tuple, list)):
        raise ValueError(f"want must be a tuple / list of names out of {MATCH_NAMES}, got {want!r}")
    for w in want:
        if w not in MATCH_NAMES:
            raise ValueError(f"want: unknown entry {w!r} (known: {MATCH_NAMES})")
    return tuple(want)


def check_taus(taus, have_freqs: bool):
    """``taus`` as ``None`` or the host triple ``(float tau0, float dtau, int n_tau)``: two finite floats and ``1 <= n_tau <=
    MATCH_MAX_TAU``, which needs the frequencies; anything else is a ValueError."""
    if taus is None:
        return None
    if isinstance(taus, torch.Tensor) or not isinstance(taus, (tuple, list)) or len(taus) != 3:
        raise ValueError(f"taus must be None or a host triple (tau0, dtau, n_tau), got {taus!r}")
    if not have_freqs:
        raise ValueError("taus (a time-shift grid) needs freqs, the physical frequency of every point")
    t0, dt, n = taus
    if any(isinstance(v, (torch.Tensor, bool)) or not isinstance(v, (int, float)) for v in (t0, dt)) \
            or isinstance(n, bool) or not isinstance(n, int):
        raise ValueError(f"taus = (tau0, dtau, n_tau) takes two host floats and a host int, got {taus!r}")
    if n < 1 or n > MATCH_MAX_TAU:
        raise ValueError(f"taus: n_tau must lie in [1, {MATCH_MAX_TAU}], got {n} (no time maximisation: taus=None)")
    tau0, dtau = float(t0), float(dt)
    if not (math.isfinite(tau0) and math.isfinite(dtau)):
        raise ValueError(f"taus: tau0 and dtau must be finite, got {tau0}, {dtau}")
    return tau0, dtau, n


def check_match_args(h_shape, g, weights=None, freqs=None, taus=None, what="g (the reference waveforms)"):
    """The shapes and host values of a :func:`waveform_match` call -> ``(R, T, h_ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau)``;
    ``ValueError`` for anything that does not fit.  Reads shapes only, so it runs on tensors of any device: ``h_shape`` = [R, T, >= 2],
    ``g`` [B, T, 2] with ``R % B == 0``, ``weights`` / ``freqs`` ``None``, [T] or [B, T], ``taus`` ``None`` or a host triple
    ``(tau0, dtau, n_tau)`` of two finite floats and ``1 <= n_tau <= MATCH_MAX_TAU``, which needs ``freqs``.  ``what``: how an error
    names ``g``."""
    h_shape = tuple(h_shape)
    if len(h_shape) != 3 or h_shape[2] < 2 or h_shape[0] < 1 or h_shape[1] < 1:
        raise ValueError(f"h must have shape [R, T, >= 2] (amplitude, phase first), got {list(h_shape)}")
    R, T, ld = h_shape
    if not isinstance(g, torch.Tensor) or g.dim() != 3 or g.shape[0] < 1 or tuple(g.shape[1:]) != (T, 2):
        raise ValueError(f"{what} must have shape [B, T={T}, 2], got "
                         f"{list(g.shape) if isinstance(g, torch.Tensor) else type(g).__name__}")
    B = g.shape[0]
    if R % B != 0:
        raise ValueError(f"h holds {R} rows, g {B} tasks: R % B != 0 (row k * B + b is latent sample k of task b)")

    def rows_of(t, what):
        if t is None:
            return 1
        if not isinstance(t, torch.Tensor) or tuple(t.shape) not in ((T,), (B, T)):
            raise ValueError(f"{what} must be None or a tensor of shape [T={T}] or [B={B}, T={T}], got "
                             f"{list(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        return 1 if t.dim() == 1 else B

    wgt_rows, freq_rows = rows_of(weights, "weights"), rows_of(freqs, "freqs")
    taus = check_taus(taus, freqs is not None)
    tau0, dtau, n_tau = taus if taus is not None else (0.0, 0.0, 0)
    return R, T, ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau


def _match_workspace(device: torch.device, n_bytes: int) -> torch.Tensor:
    """The float64 workspace of the device, at least ``n_bytes`` long.  It grows outside graph capture only, and a workspace it
    outgrows is kept: a graph captured earlier still writes to it.  One workspace per device: calls from several streams of one
    device must be ordered by the caller."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    held = _MATCH_WS.setdefault(idx, [])
    need = (n_bytes + 7) // 8
    if not held or held[-1].numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("waveform_match: the workspace has to grow, which cannot happen during graph capture; call once at "
                               "these sizes before capturing")
        held.append(torch.empty((max(need, 2 * held[-1].numel() if held else 0),), dtype=torch.float64, device=device))
    return held[-1]


def waveform_match(h: torch.Tensor, g: torch.Tensor, weights: Optional[torch.Tensor] = None, freqs: Optional[torch.Tensor] = None,
                   taus=None, n_valid: Optional[torch.Tensor] = None, want=MATCH_NAMES, corr: bool = False) -> WaveformMatch:
    """Overlap, match and mismatch of the predicted waveforms ``h`` [R, T, >= 2] (amplitude ``h[..., 0]``, phase ``h[..., 1]``; any
    contiguous fp32 device tensor, e.g. the raw decoder output of a ``dy = 2`` head) against the reference waveforms ``g`` [B, T, 2],
    row ``k * B + b`` of ``h`` against task ``b``: the weighted complex correlation ``c_j = sum_t w A A' exp(i (phi - phi' + 2 pi f
    tau_j))`` over the uniform grid ``tau_j = tau0 + j dtau`` of ``taus = (tau0, dtau, n_tau)``, normalised by ``sqrt(hh gg)``;
    ``match = max_j |c_j|`` with ``tau_index`` the first index that attains it and ``phase = arg c`` there, ``overlap`` the real part
    without time shift, ``mismatch = 1 - match`` formed in double (``include/npf_hip.h`` has the formulae and the edge cases).
    ``taus=None``: no time maximisation (``match = |c|`` without shift, ``tau_index = 0``).  ``weights`` (``4 df / S_n(f)``; ``None``:
    ones) and ``freqs`` (Hz): [T], shared by the tasks, or [B, T]; a point whose weight is not in (0, inf) is removed, whatever the
    other tensors hold there.  ``n_valid``: device integer tensor [B], the real points of every task.  ``want``: the names out of
    ``MATCH_NAMES`` to compute; ``corr=True`` adds the normalised correlation over the whole grid [R, max(n_tau, 1), 2].  Two
    ``npf_waveform_match`` launches in double arithmetic, inference only (no autograd), no host sync, deterministic; the workspace
    is cached per device."""
    want = check_match_want(want)
    R, T, ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau = check_match_args(getattr(h, "shape", ()), g, weights, freqs, taus)
    if not want and not corr:
        raise ValueError(f"want must name at least one of {MATCH_NAMES} (or corr=True)")
    for t in (h, g, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    h, g = h.detach().contiguous(), g.detach().contiguous()
    weights = weights.detach().contiguous() if weights is not None else None
    freqs = freqs.detach().contiguous() if freqs is not None and n_tau > 0 else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    return _match_launch(h, g, weights, freqs, nv, (R, T, ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau), want, corr, None)


def _match_launch(h, g, weights, freqs, nv, geo, want, corr, saved) -> WaveformMatch:
    """The two forward launches on prepared (detached, contiguous) tensors; ``saved``: ``None`` or the float64 [R, 4] tensor that
    takes the unrounded row scalars (``npf_waveform_match_ex``)."""
    R, T, ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau = geo
    lib = L.load()
    ws = _match_workspace(h.device, int(lib.npf_waveform_match_workspace_bytes(R, n_tau)))
    new = lambda n, dtype=torch.float32: torch.empty((n,), dtype=dtype, device=h.device)  # noqa: E731
    out = {name: (new(B if name == "gg" else R, torch.int32 if name == "tau_index" else torch.float32) if name in want else None)
           for name in MATCH_NAMES}
    c = torch.empty((R, max(n_tau, 1), 2), dtype=torch.float32, device=h.device) if corr else None
    args = (L.ptr(h), ld, L.ptr(g), L.ptr(weights), wgt_rows, L.ptr(freqs), freq_rows, _iptr(nv) if nv is not None else None, R, B, T,
            tau0, dtau, n_tau, *(out[name].data_ptr() if out[name] is not None else None for name in MATCH_NAMES), L.ptr(c),
            ws.data_ptr())
    if saved is None:
        L.check(lib.npf_waveform_match(*args, L.stream_ptr()), "npf_waveform_match")
    else:
        L.check(lib.npf_waveform_match_ex(*args, saved.data_ptr(), L.stream_ptr()), "npf_waveform_match_ex")
    return WaveformMatch(*(out[name] for name in MATCH_NAMES), c)


# ---- bank match: every row against every template of one shared bank (csrc/waveform_bank_kernels.hip) ----
BANK_NAMES = ("hh", "gg", "match", "mismatch", "tau_index", "phase", "best_index", "best_match")
BANK_MAX_ROWS = 1 << 24
BANK_MAX_BANK = 1 << 20


class WaveformBankMatch(NamedTuple):
    """What :func:`waveform_match_bank` returns; the entries that were not asked for are ``None``."""
    hh: Optional[torch.Tensor]          # [R] sum_t w A^2
    gg: Optional[torch.Tensor]          # [G] sum_t w A'^2
    match: Optional[torch.Tensor]       # [R, G]
    mismatch: Optional[torch.Tensor]    # [R, G]
    tau_index: Optional[torch.Tensor]   # [R, G] int32
    phase: Optional[torch.Tensor]       # [R, G]
    best_index: Optional[torch.Tensor]  # [R] int32: the template of the largest match, the smallest index
    best_match: Optional[torch.Tensor]  # [R] the match there
    dot: Optional[torch.Tensor]         # [R, G, 2] float64: the unrounded correlation at the maximum (``dot=True``)


def check_bank_want(want) -> tuple:
    """``want`` as a tuple of names out of ``BANK_NAMES`` (may be empty: ``dot`` alone); anything else is a ValueError."""
    if isinstance(want, str) or not isinstance(want, (tuple, list)):
        raise ValueError(f"want must be a tuple / list of names out of {BANK_NAMES}, got {want!r}")
    for w in want:
        if w not in BANK_NAMES:
            raise ValueError(f"want: unknown entry {w!r} (known: {BANK_NAMES})")
    return tuple(want)


def check_match_bank_args(h_shape, bank, weights=None, freqs=None, taus=None):
    """The shapes and host values of a :func:`waveform_match_bank` call -> ``(R, T, h_ld, G, tau0, dtau, n_tau)``; ``ValueError`` for
    anything that does not fit.  Reads shapes only, so it runs on tensors of any device: ``h_shape`` = [R, T, >= 2] with ``R <=
    BANK_MAX_ROWS``, ``bank`` [G, T, 2] with ``G <= BANK_MAX_BANK``, ``weights`` / ``freqs`` ``None`` or [T] -- the bank is shared
    by the rows, so there is one frequency grid -- and ``taus`` as in :func:`check_match_args`."""
    h_shape = tuple(h_shape)
    if len(h_shape) != 3 or h_shape[2] < 2 or h_shape[0] < 1 or h_shape[1] < 1:
        raise ValueError(f"h must have shape [R, T, >= 2] (amplitude, phase first), got {list(h_shape)}")
    R, T, ld = h_shape
    if R > BANK_MAX_ROWS:
        raise ValueError(f"h holds {R} rows; a bank match takes at most {BANK_MAX_ROWS}")
    if not isinstance(bank, torch.Tensor) or bank.dim() != 3 or bank.shape[0] < 1 or tuple(bank.shape[1:]) != (T, 2):
        raise ValueError(f"bank must have shape [G, T={T}, 2], got "
                         f"{list(bank.shape) if isinstance(bank, torch.Tensor) else type(bank).__name__}")
    G = bank.shape[0]
    if G > BANK_MAX_BANK:
        raise ValueError(f"bank holds {G} templates; a bank match takes at most {BANK_MAX_BANK}")
    for t, what in ((weights, "weights"), (freqs, "freqs")):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (T,)):
            raise ValueError(f"{what} must be None or a tensor of shape [T={T}] (one grid shared by the bank), got "
                             f"{list(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    taus = check_taus(taus, freqs is not None)
    tau0, dtau, n_tau = taus if taus is not None else (0.0, 0.0, 0)
    return R, T, ld, G, tau0, dtau, n_tau


def waveform_match_bank(h: torch.Tensor, bank: torch.Tensor, weights: Optional[torch.Tensor] = None,
                        freqs: Optional[torch.Tensor] = None, taus=None, want=BANK_NAMES, dot: bool = False) -> WaveformBankMatch:
    """The match of EVERY predicted waveform ``h`` [R, T, >= 2] (amplitude, phase first) against EVERY template of ``bank``
    [G, T, 2], one bank shared by the rows: ``c_j[r, g] = sum_t w A A' exp(i (phi - phi' + 2 pi f tau_j))`` over the grid of ``taus
    = (tau0, dtau, n_tau)``, ``match[r, g] = max_j |c_j| / sqrt(hh_r gg_g)`` with ``tau_index`` the first index that attains it and
    ``phase = arg c`` there, ``mismatch = 1 - match`` formed in double; ``best_index[r]`` is the template of the largest match that is
    not NaN (the smallest index; 0 if there is none) and ``best_match[r]`` the match there.  ``weights`` (``None``: ones) and
    ``freqs`` are [T]: a shared bank means a shared grid; a point whose weight is not in (0, inf) is removed, whatever the other
    tensors hold there.  ``want``: the names out of ``BANK_NAMES`` to compute; ``dot=True`` adds the correlation at the maximum as
    unrounded float64 [R, G, 2].  ``npf_waveform_match_bank``: the per-shift rotation is done once per row and the contraction runs
    on the double-precision matrix instruction (``include/npf_hip.h`` has the contract); inference only (no autograd), no host sync,
    deterministic; the workspace is the one of :func:`waveform_match`."""
    want = check_bank_want(want)
    R, T, ld, G, tau0, dtau, n_tau = check_match_bank_args(getattr(h, "shape", ()), bank, weights, freqs, taus)
    if not want and not dot:
        raise ValueError(f"want must name at least one of {BANK_NAMES} (or dot=True)")
    for t in (h, bank, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    h, bank = h.detach().contiguous(), bank.detach().contiguous()
    weights = weights.detach().contiguous() if weights is not None else None
    freqs = freqs.detach().contiguous() if freqs is not None and n_tau > 0 else None
    lib = L.load()
    ws = _match_workspace(h.device, int(lib.npf_waveform_match_bank_workspace_bytes(R, G, T, n_tau)))
    shape = {"hh": (R,), "gg": (G,), "best_index": (R,), "best_match": (R,)}
    out = {name: (torch.empty(shape.get(name, (R, G)), dtype=torch.int32 if name.endswith("index") else torch.float32, device=h.device)
                  if name in want else None) for name in BANK_NAMES}
    d = torch.empty((R, G, 2), dtype=torch.float64, device=h.device) if dot else None
    ptr = lambda name: out[name].data_ptr() if out[name] is not None else None  # noqa: E731
    L.check(lib.npf_waveform_match_bank(L.ptr(h), ld, L.ptr(bank), L.ptr(weights), L.ptr(freqs), R, G, T, tau0, dtau, n_tau,
                                        ptr("hh"), ptr("gg"), ptr("match"), ptr("mismatch"), ptr("tau_index"), ptr("phase"),
                                        d.data_ptr() if d is not None else None, ptr("best_index"), ptr("best_match"), ws.data_ptr(),
                                        L.stream_ptr()), "npf_waveform_match_bank")
    return WaveformBankMatch(*(out[name] for name in BANK_NAMES), d)


class _WaveformMismatchFn(torch.autograd.Function):
    """``mismatch`` [R] of the rows of ``h_eval`` against ``g`` (``npf_waveform_match_ex``, which keeps the unrounded row scalars) and
    its gradient with respect to ``src`` (``npf_waveform_match_bwd``, one launch that writes every element): ``src`` is ``h_eval``
    itself (``n_bcast`` = 1) or the [n_bcast * R, T, ld] samples whose mean over the ``n_bcast`` row blocks ``h_eval`` holds."""

    @staticmethod
    def forward(ctx, src, h_eval, g, weights, freqs, nv, geo, n_bcast):
        R = geo[0]
        saved = torch.empty((R, 4), dtype=torch.float64, device=h_eval.device)
        m = _match_launch(h_eval, g, weights, freqs, nv, geo, ("mismatch", "tau_index"), False, saved)
        ctx.save_for_backward(h_eval, g, weights, freqs, nv, m.tau_index, saved)
        ctx.cfg = (geo, n_bcast, tuple(src.shape))
        ctx.mark_non_differentiable(m.tau_index)
        return m.mismatch, m.tau_index

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_mismatch, _):
        h_eval, g, weights, freqs, nv, tau_index, saved = ctx.saved_tensors
        (R, T, ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau), n_bcast, src_shape = ctx.cfg
        d_match = d_mismatch.neg().contiguous()  # (mismatch = 1 - match)
        d_src = torch.empty(src_shape, dtype=torch.float32, device=h_eval.device)  # (written whole: no memset)
        L.check(L.load().npf_waveform_match_bwd(L.ptr(h_eval), ld, L.ptr(g), L.ptr(weights), wgt_rows, L.ptr(freqs), freq_rows,
                                                _iptr(nv) if nv is not None else None, R, B, T, tau0, dtau, n_tau, _iptr(tau_index),
                                                saved.data_ptr(), L.ptr(d_match), n_bcast, L.ptr(d_src), src_shape[2],
                                                L.stream_ptr()), "npf_waveform_match_bwd")
        return d_src, None, None, None, None, None, None, None


def waveform_mismatch(h: torch.Tensor, g: torch.Tensor, weights: Optional[torch.Tensor] = None, freqs: Optional[torch.Tensor] = None,
                      taus=None, n_valid: Optional[torch.Tensor] = None, n_bcast: int = 1,
                      mean: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mismatch`` [R] of :func:`waveform_match` (same arguments, same bits), differentiable with respect to ``h``: the training
    objective that sees a phase error coherent across the band.  The forward is the two launches of ``npf_waveform_match_ex``, which
    also keeps ``(hh, gg, c_{j*})`` in double, the backward one ``npf_waveform_match_bwd`` launch that writes the whole gradient of
    ``h`` [.., T, ld]: entries 0 and 1 of a point get ``-dM/dA`` and ``-dM/dphi`` (``include/npf_hip.h`` has the formulae), entries
    2 .. ld - 1 (the raw scale of a decoder row), removed and padded points and degenerate rows get exact zeros.  The derivative is
    taken at the grid time the forward found (Danskin); where two grid times tie it is the derivative at the smaller index, a
    subgradient.  There is no gradient with respect to ``g``, ``weights`` or ``freqs``: one of them with ``requires_grad`` is a
    ``ValueError``.  No double backward.  ``n_bcast`` > 1: ``h`` [n_bcast * R, T, ld] holds ``n_bcast`` latent samples of every row
    (row ``q * R + r``) and ``mean`` [R, T, >= 2] their mean (e.g. of :func:`mixture_summary`; required then, and accepted with
    ``n_bcast`` = 1 as the mean of one sample), on which the mismatch is evaluated;
    the mean is linear, so every sample receives ``1 / n_bcast`` of the row's gradient.  No host sync; the workspace is the one of
    :func:`waveform_match`, so inside a captured graph the call needs one earlier call at these sizes."""
    if isinstance(n_bcast, bool) or not isinstance(n_bcast, int) or n_bcast < 1:
        raise ValueError(f"n_bcast must be a host int >= 1, got {n_bcast!r}")
    if n_bcast > 1 and mean is None:
        raise ValueError("n_bcast > 1 evaluates the mismatch on `mean`, the mean of the n_bcast samples h holds: give it")
    h_shape = tuple(getattr(h, "shape", ()))
    if mean is not None:
        if len(h_shape) != 3 or h_shape[0] % n_bcast != 0 or h_shape[2] < 2:
            raise ValueError(f"h must have shape [n_bcast * R, T, >= 2] with n_bcast={n_bcast}, got {list(h_shape)}")
        if not isinstance(mean, torch.Tensor) or mean.dim() != 3 or tuple(mean.shape[:2]) != (h_shape[0] // n_bcast, h_shape[1]):
            raise ValueError(f"mean must have shape [R={h_shape[0] // n_bcast}, T={h_shape[1]}, >= 2], got "
                             f"{list(mean.shape) if isinstance(mean, torch.Tensor) else type(mean).__name__}")
    h_eval = h if mean is None else mean
    geo = check_match_args(getattr(h_eval, "shape", ()), g, weights, freqs, taus)
    for t, what in ((g, "g"), (weights, "weights"), (freqs, "freqs")):
        if t is not None and t.requires_grad:
            raise ValueError(f"waveform_mismatch has no gradient with respect to {what}: detach it")
    for t in (h, mean, g, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    n_tau, B = geo[8], geo[3]
    h = h.contiguous()
    h_eval = h.detach() if mean is None else mean.detach().contiguous()
    weights = weights.detach().contiguous() if weights is not None else None
    freqs = freqs.detach().contiguous() if freqs is not None and n_tau > 0 else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    return _WaveformMismatchFn.apply(h, h_eval, g.detach().contiguous(), weights, freqs, nv, geo, n_bcast)[0]


# ---- matched-filter log likelihood of complex data (csrc/waveform_kernels.hip) --------------
LOGLIKE_NAMES = ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "lnl_mix", "lnl_max_mix")
LOGLIKE_I0_SWITCH = 24.0  # ln I0(x): power series below, the 1 / (8 x) series from here on (NPF_LOGLIKE_I0_SWITCH)
_LOGLIKE_PER_TASK = ("dd", "lnl_mix", "lnl_max_mix")


class WaveformLogLike(NamedTuple):
    """What :func:`waveform_loglike` returns (float64 but ``tau_index``); the entries that were not asked for are ``None``."""
    hh: Optional[torch.Tensor]           # [R] sum_t w A^2: the optimal SNR squared
    dd: Optional[torch.Tensor]           # [B] sum_t w |d|^2
    snr: Optional[torch.Tensor]          # [R] max_j |kappa_j| / sqrt(hh)
    lnl_max: Optional[torch.Tensor]      # [R] phase and time maximised
    lnl_marg: Optional[torch.Tensor]     # [R] phase and time marginalised
    tau_index: Optional[torch.Tensor]    # [R] int32
    phase: Optional[torch.Tensor]        # [R]
    lnl_mix: Optional[torch.Tensor]      # [B] lnl_marg marginalised over the latent samples
    lnl_max_mix: Optional[torch.Tensor]  # [B] the same of lnl_max
    series: Optional[torch.Tensor]       # [R, max(n_tau, 1), 2] = (L_j, x_j / sqrt(hh))


def check_loglike_args(h_shape, data, weights=None, freqs=None, taus=None):
    """The shapes and host values of a :func:`waveform_loglike` call -> what :func:`check_match_args` returns, under its rules:
    ``data`` [B, T, 2] = (Re, Im) stands where its ``g`` stands.  Reads shapes only."""
    return check_match_args(h_shape, data, weights, freqs, taus, what="data = (Re, Im)")


def waveform_loglike(h: torch.Tensor, data: torch.Tensor, weights: Optional[torch.Tensor] = None, freqs: Optional[torch.Tensor] = None,
                     taus=None, n_valid: Optional[torch.Tensor] = None, want=LOGLIKE_NAMES, series: bool = False) -> WaveformLogLike:
    """Matched-filter SNR and log likelihood ratio of the complex data ``data`` [B, T, 2] = (Re d, Im d) under the predicted
    waveforms ``h`` [R, T, >= 2] (amplitude, phase first; row ``s * B + b`` is latent sample ``s`` of task ``b``): with
    ``kappa_j = sum_t w A e^{i (phi + 2 pi f tau_j)} conj(d)`` over the grid of ``taus = (tau0, dtau, n_tau)`` and ``hh = sum_t w A^2``,
    ``snr = max_j |kappa_j| / sqrt(hh)`` with ``tau_index`` the first index that attains it and ``phase = arg kappa`` there,
    ``lnl_max = max_j |kappa_j| - hh / 2``, ``lnl_marg = logsumexp_j (ln I0(|kappa_j|) - hh / 2) - ln n_tau`` and per task the
    log-mean-exp of both over the ``R / B`` latent samples (``lnl_mix``, ``lnl_max_mix``); ``include/npf_hip.h`` has the contract and
    the edge cases.  ``-dd / 2`` is added to nothing.  ``weights``, ``freqs``, ``taus``, ``n_valid``: as in :func:`waveform_match`.
    ``want``: the names out of ``LOGLIKE_NAMES`` to compute; ``series=True`` adds ``(L_j, x_j / sqrt(hh))`` over the whole grid.
    Every result is float64.  Two ``npf_waveform_loglike`` launches in double arithmetic, inference only, no host sync,
    deterministic; the workspace is the one of :func:`waveform_match`."""
    if isinstance(want, str) or not isinstance(want, (tuple, list)) or any(w not in LOGLIKE_NAMES for w in want):
        raise ValueError(f"want must be a tuple / list of names out of {LOGLIKE_NAMES}, got {want!r}")
    want = tuple(want)
    R, T, ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau = check_loglike_args(getattr(h, "shape", ()), data, weights, freqs, taus)
    if not want and not series:
        raise ValueError(f"want must name at least one of {LOGLIKE_NAMES} (or series=True)")
    for t in (h, data, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    h, data = h.detach().contiguous(), data.detach().contiguous()
    weights = weights.detach().contiguous() if weights is not None else None
    freqs = freqs.detach().contiguous() if freqs is not None and n_tau > 0 else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    lib = L.load()
    ws = _match_workspace(h.device, int(lib.npf_waveform_loglike_workspace_bytes(R, n_tau)))
    out = {name: (torch.empty((B if name in _LOGLIKE_PER_TASK else R,), dtype=torch.int32 if name == "tau_index" else torch.float64,
                              device=h.device) if name in want else None) for name in LOGLIKE_NAMES}
    ser = torch.empty((R, max(n_tau, 1), 2), dtype=torch.float64, device=h.device) if series else None
    dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    per_row = [dptr(out[name]) for name in ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase")]
    L.check(lib.npf_waveform_loglike(L.ptr(h), ld, L.ptr(data), L.ptr(weights), wgt_rows, L.ptr(freqs), freq_rows,
                                     _iptr(nv) if nv is not None else None, R, B, T, tau0, dtau, n_tau, *per_row, dptr(ser),
                                     dptr(out["lnl_mix"]), dptr(out["lnl_max_mix"]), ws.data_ptr(), L.stream_ptr()),
            "npf_waveform_loglike")
    return WaveformLogLike(*(out[name] for name in LOGLIKE_NAMES), ser)


# ---- coherent matched-filter log likelihood of a detector network (csrc/waveform_net_kernels.hip) --------------
NET_MAX_DET = 8  # NPF_NET_MAX_DET
LOGLIKE_NET_NAMES = LOGLIKE_NAMES + ("hh_det", "snr_det", "dd_det")
_LOGLIKE_NET_PER_DET = ("hh_det", "snr_det", "dd_det")


class WaveformLogLikeNetwork(NamedTuple):
    """What :func:`waveform_loglike_network` returns (float64 but ``tau_index``); the entries that were not asked for are ``None``."""
    hh: Optional[torch.Tensor]           # [R] HH = sum_k |C_k|^2 hh_k: the optimal network SNR squared
    dd: Optional[torch.Tensor]           # [B] DD = sum_k dd_k
    snr: Optional[torch.Tensor]          # [R] max_j |K_j| / sqrt(HH)
    lnl_max: Optional[torch.Tensor]      # [R] phase and time maximised
    lnl_marg: Optional[torch.Tensor]     # [R] phase and time marginalised
    tau_index: Optional[torch.Tensor]    # [R] int32
    phase: Optional[torch.Tensor]        # [R]
    lnl_mix: Optional[torch.Tensor]      # [B] lnl_marg marginalised over the latent samples
    lnl_max_mix: Optional[torch.Tensor]  # [B] the same of lnl_max
    hh_det: Optional[torch.Tensor]       # [R, D] hh_k = sum_t w_k A^2
    snr_det: Optional[torch.Tensor]      # [R, D] |kappa_{k,j*}| / sqrt(hh_k) at the network's grid time
    dd_det: Optional[torch.Tensor]       # [B, D] dd_k = sum_t w_k |d_k|^2
    series: Optional[torch.Tensor]       # [R, max(n_tau, 1), 2] = (L_j, x_j / sqrt(HH))


def check_loglike_network_args(h_shape, data, response, delays=None, weights=None, freqs=None, taus=None):
    """The shapes, dtypes and host values of a :func:`waveform_loglike_network` call -> ``(R, T, h_ld, B, D, wgt_rows, freq_rows, tau0,
    dtau, n_tau)``; ``ValueError`` for anything that does not fit.  Reads shapes and dtypes only, so it runs on tensors of any
    device: ``h_shape`` = [R, T, >= 2], ``data`` [B, D, T, 2] with ``1 <= D <= NET_MAX_DET`` and ``R % B == 0``, ``response``
    float64 [B, D, 2], ``delays`` ``None`` or float64 [B, D] (needs ``freqs``), ``weights`` ``None``, [D, T] or [B, D, T], ``freqs``
    ``None``, [T] or [B, T], ``taus`` as in :func:`check_match_args`."""
    h_shape = tuple(h_shape)
    if len(h_shape) != 3 or h_shape[2] < 2 or h_shape[0] < 1 or h_shape[1] < 1:
        raise ValueError(f"h must have shape [R, T, >= 2] (amplitude, phase first), got {list(h_shape)}")
    R, T, ld = h_shape
    shape_of = lambda t: list(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__  # noqa: E731
    if not isinstance(data, torch.Tensor) or data.dim() != 4 or data.shape[0] < 1 or tuple(data.shape[2:]) != (T, 2):
        raise ValueError(f"data = (Re, Im) per detector must have shape [B, D, T={T}, 2], got {shape_of(data)}")
    B, D = data.shape[0], data.shape[1]
    if not 1 <= D <= NET_MAX_DET:
        raise ValueError(f"data holds {D} detectors: 1 <= D <= {NET_MAX_DET}")
    if R % B != 0:
        raise ValueError(f"h holds {R} rows, data {B} tasks: R % B != 0 (row k * B + b is latent sample k of task b)")
    if not isinstance(response, torch.Tensor) or tuple(response.shape) != (B, D, 2) or response.dtype != torch.float64:
        raise ValueError(f"response = (Re C, Im C) must be a float64 tensor of shape [B={B}, D={D}, 2], got {shape_of(response)}"
                         f"{' of ' + str(response.dtype) if isinstance(response, torch.Tensor) else ''}")
    if delays is not None and (not isinstance(delays, torch.Tensor) or tuple(delays.shape) != (B, D) or delays.dtype != torch.float64):
        raise ValueError(f"delays (seconds) must be None or a float64 tensor of shape [B={B}, D={D}], got {shape_of(delays)}"
                         f"{' of ' + str(delays.dtype) if isinstance(delays, torch.Tensor) else ''}")
    if weights is not None and (not isinstance(weights, torch.Tensor) or tuple(weights.shape) not in ((D, T), (B, D, T))):
        raise ValueError(f"weights must be None or a tensor of shape [D={D}, T={T}] or [B={B}, D={D}, T={T}], got {shape_of(weights)}")
    if freqs is not None and (not isinstance(freqs, torch.Tensor) or tuple(freqs.shape) not in ((T,), (B, T))):
        raise ValueError(f"freqs must be None or a tensor of shape [T={T}] or [B={B}, T={T}], got {shape_of(freqs)}")
    if delays is not None and freqs is None:
        raise ValueError("delays need freqs: a delay enters as the phase 2 pi f delay")
    wgt_rows = 1 if weights is None or weights.dim() == 2 else B
    freq_rows = 1 if freqs is None or freqs.dim() == 1 else B
    taus = check_taus(taus, freqs is not None)
    tau0, dtau, n_tau = taus if taus is not None else (0.0, 0.0, 0)
    return R, T, ld, B, D, wgt_rows, freq_rows, tau0, dtau, n_tau


def waveform_loglike_network(h: torch.Tensor, data: torch.Tensor, response: torch.Tensor, delays: Optional[torch.Tensor] = None,
                             weights: Optional[torch.Tensor] = None, freqs: Optional[torch.Tensor] = None, taus=None,
                             n_valid: Optional[torch.Tensor] = None, want=LOGLIKE_NET_NAMES,
                             series: bool = False) -> WaveformLogLikeNetwork:
    """Coherent matched-filter SNR and log likelihood ratio of the data of a network of ``D`` detectors, ``data`` [B, D, T, 2] =
    (Re d_k, Im d_k), under the predicted waveforms ``h`` [R, T, >= 2] (as in :func:`waveform_loglike`).  Detector ``k`` sees
    ``C_k h`` shifted by ``tau_j + delay_k``: ``response`` [B, D, 2] = (Re C, Im C) and ``delays`` [B, D] (seconds, either sign, not
    tied to the grid; ``None``: zeros) are float64 DEVICE tensors, taken as they are -- the host does not read them, so a captured
    graph sees what they hold at replay.  With ``kappa_{k,j} = sum_t w_k A e^{i (phi + 2 pi f (tau_j + delay_k))} conj(d_k)`` the
    network sums ``K_j = sum_k C_k kappa_{k,j}``, ``HH = sum_k |C_k|^2 hh_k``, ``DD = sum_k dd_k`` stand where ``kappa_j``, ``hh``,
    ``dd`` stand in :func:`waveform_loglike`: the complex correlations are added before the modulus is taken, one phase and one
    arrival time are shared by the detectors.  ``hh_det`` / ``dd_det`` are the detectors' own ``hh_k`` / ``dd_k`` and ``snr_det``
    is ``|kappa_{k,j*}| / sqrt(hh_k)`` at the network's grid time; ``include/npf_hip.h`` has the contract and the edge cases.
    ``weights``: [D, T] or [B, D, T] (``None``: ones); a point is removed per detector.  ``freqs`` ([T] or [B, T]) is shared by the
    detectors and required with ``taus`` or ``delays``.  ``taus``, ``n_valid``, ``want`` (names out of ``LOGLIKE_NET_NAMES``),
    ``series``: as in :func:`waveform_loglike`.  Two ``npf_waveform_loglike_net`` launches in double arithmetic, inference only,
    no host sync, deterministic; the workspace is the one of :func:`waveform_match`."""
    if isinstance(want, str) or not isinstance(want, (tuple, list)) or any(w not in LOGLIKE_NET_NAMES for w in want):
        raise ValueError(f"want must be a tuple / list of names out of {LOGLIKE_NET_NAMES}, got {want!r}")
    want = tuple(want)
    R, T, ld, B, D, wgt_rows, freq_rows, tau0, dtau, n_tau = check_loglike_network_args(getattr(h, "shape", ()), data, response, delays,
                                                                                        weights, freqs, taus)
    if not want and not series:
        raise ValueError(f"want must name at least one of {LOGLIKE_NET_NAMES} (or series=True)")
    for t in (h, data, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    for t, what in ((response, "response"), (delays, "delays")):
        if t is not None and (not t.is_cuda or t.device != h.device):
            raise ValueError(f"{what} must live on the device of h ({h.device}), got {t.device}: the kernel reads it there")
    h, data = h.detach().contiguous(), data.detach().contiguous()
    response = response.detach().contiguous()
    delays = delays.detach().contiguous() if delays is not None else None
    weights = weights.detach().contiguous() if weights is not None else None
    freqs = freqs.detach().contiguous() if freqs is not None and (n_tau > 0 or delays is not None) else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    lib = L.load()
    ws = _match_workspace(h.device, int(lib.npf_waveform_loglike_net_workspace_bytes(R, D, n_tau)))

    def new(name):
        rows = B if name in _LOGLIKE_PER_TASK or name == "dd_det" else R
        return torch.empty((rows, D) if name in _LOGLIKE_NET_PER_DET else (rows,),
                           dtype=torch.int32 if name == "tau_index" else torch.float64, device=h.device)

    out = {name: (new(name) if name in want else None) for name in LOGLIKE_NET_NAMES}
    ser = torch.empty((R, max(n_tau, 1), 2), dtype=torch.float64, device=h.device) if series else None
    dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    per_row = [dptr(out[name]) for name in ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase")]
    L.check(lib.npf_waveform_loglike_net(L.ptr(h), ld, L.ptr(data), L.ptr(weights), wgt_rows, L.ptr(freqs), freq_rows,
                                         _iptr(nv) if nv is not None else None, dptr(delays), dptr(response), R, B, D, T, tau0, dtau,
                                         n_tau, *per_row, dptr(ser), dptr(out["lnl_mix"]), dptr(out["lnl_max_mix"]),
                                         dptr(out["hh_det"]), dptr(out["snr_det"]), dptr(out["dd_det"]), ws.data_ptr(),
                                         L.stream_ptr()), "npf_waveform_loglike_net")
    return WaveformLogLikeNetwork(*(out[name] for name in LOGLIKE_NET_NAMES), ser)


# ---- sky-grid network likelihood (csrc/waveform_sky_kernels.hip) --------------
SKY_MAX_PIX = 65536  # NPF_SKY_MAX_PIX
SKY_JC = 8           # NPF_SKY_JC: time shifts per chunk of the correlation launch
LOGLIKE_SKY_NAMES = ("lnl_sky", "pix_index", "tau_index", "snr", "lnl_sky_mix")


class WaveformLogLikeSky(NamedTuple):
    """What :func:`waveform_loglike_sky` returns (float64 but the two indices); the entries that were not asked for are ``None``."""
    lnl_sky: Optional[torch.Tensor]      # [R] phase, time and sky position marginalised
    pix_index: Optional[torch.Tensor]    # [R] int32: the pixel of the largest evidence, the smallest index
    tau_index: Optional[torch.Tensor]    # [R] int32: the grid time of the largest |K_j| at that pixel
    snr: Optional[torch.Tensor]          # [R] max_j |K_j| / sqrt(HH) at that pixel
    lnl_sky_mix: Optional[torch.Tensor]  # [B] lnl_sky marginalised over the latent samples
    post: Optional[torch.Tensor]         # [R, P] log posterior mass of every pixel (``posterior=True``)
    post_mix: Optional[torch.Tensor]     # [B, P] the same with the latent samples marginalised (``posterior=True``)
    snr_map: Optional[torch.Tensor]      # [R, P] max_j |K_j| / sqrt(HH) of every pixel (``snr_map=True``)


def check_loglike_sky_args(h_shape, data, response, delays, log_prior=None, weights=None, freqs=None, taus=None):
    """The shapes, dtypes and host values of a :func:`waveform_loglike_sky` call -> ``(R, T, h_ld, B, D, P, wgt_rows, tau0, dtau,
    n_tau)``; ``ValueError`` for anything that does not fit.  Reads shapes and dtypes only, so it runs on tensors of any device:
    ``h_shape`` = [R, T, >= 2], ``data`` [B, D, T, 2] with ``1 <= D <= NET_MAX_DET`` and ``R % B == 0``, ``response`` float64
    [P, D, 2] with ``1 <= P <= SKY_MAX_PIX``, ``delays`` float64 [P, D], ``log_prior`` ``None`` or float64 [P], ``weights``
    ``None``, [D, T] or [B, D, T], ``freqs`` [T] -- required, and one row: the sky grid is shared by the tasks, so [B, T] is refused
    -- and ``taus`` as in :func:`check_match_args`."""
    h_shape = tuple(h_shape)
    if len(h_shape) != 3 or h_shape[2] < 2 or h_shape[0] < 1 or h_shape[1] < 1:
        raise ValueError(f"h must have shape [R, T, >= 2] (amplitude, phase first), got {list(h_shape)}")
    R, T, ld = h_shape
    shape_of = lambda t: (f"{list(t.shape)} of {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__)  # noqa: E731
    if not isinstance(data, torch.Tensor) or data.dim() != 4 or data.shape[0] < 1 or tuple(data.shape[2:]) != (T, 2):
        raise ValueError(f"data = (Re, Im) per detector must have shape [B, D, T={T}, 2], got {shape_of(data)}")
    B, D = data.shape[0], data.shape[1]
    if not 1 <= D <= NET_MAX_DET:
        raise ValueError(f"data holds {D} detectors: 1 <= D <= {NET_MAX_DET}")
    if R % B != 0:
        raise ValueError(f"h holds {R} rows, data {B} tasks: R % B != 0 (row k * B + b is latent sample k of task b)")
    if not isinstance(response, torch.Tensor) or response.dim() != 3 or tuple(response.shape[1:]) != (D, 2) \
            or response.dtype != torch.float64:
        raise ValueError(f"response = (Re C, Im C) per pixel must be a float64 tensor of shape [P, D={D}, 2], got {shape_of(response)}")
    P = response.shape[0]
    if not 1 <= P <= SKY_MAX_PIX:
        raise ValueError(f"response holds {P} pixels: 1 <= P <= {SKY_MAX_PIX}")
    if not isinstance(delays, torch.Tensor) or tuple(delays.shape) != (P, D) or delays.dtype != torch.float64:
        raise ValueError(f"delays (seconds) per pixel must be a float64 tensor of shape [P={P}, D={D}], got {shape_of(delays)}")
    if log_prior is not None and (not isinstance(log_prior, torch.Tensor) or tuple(log_prior.shape) != (P,)
                                  or log_prior.dtype != torch.float64):
        raise ValueError(f"log_prior must be None or a float64 tensor of shape [P={P}], got {shape_of(log_prior)}")
    if weights is not None and (not isinstance(weights, torch.Tensor) or tuple(weights.shape) not in ((D, T), (B, D, T))):
        raise ValueError(f"weights must be None or a tensor of shape [D={D}, T={T}] or [B={B}, D={D}, T={T}], got {shape_of(weights)}")
    if freqs is None:
        raise ValueError("freqs is required: the delays of a pixel enter as the phase 2 pi f delay")
    if not isinstance(freqs, torch.Tensor) or tuple(freqs.shape) != (T,):
        raise ValueError(f"freqs must be a tensor of shape [T={T}] (one grid: the sky grid is shared by the tasks), got {shape_of(freqs)}")
    wgt_rows = 1 if weights is None or weights.dim() == 2 else B
    taus = check_taus(taus, True)
    tau0, dtau, n_tau = taus if taus is not None else (0.0, 0.0, 0)
    return R, T, ld, B, D, P, wgt_rows, tau0, dtau, n_tau


def waveform_loglike_sky(h: torch.Tensor, data: torch.Tensor, response: torch.Tensor, delays: torch.Tensor,
                         log_prior: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                         freqs: Optional[torch.Tensor] = None, taus=None, n_valid: Optional[torch.Tensor] = None,
                         want=LOGLIKE_SKY_NAMES, posterior: bool = False, snr_map: bool = False) -> WaveformLogLikeSky:
    """The coherent network likelihood of :func:`waveform_loglike_network` at every pixel of ONE sky grid shared by the tasks, and
    its marginal over the pixels.  ``response`` [P, D, 2] = (Re C, Im C), ``delays`` [P, D] (seconds, either sign, not tied to the
    grid) and ``log_prior`` [P] (the log prior MASS of every pixel; ``None``: uniform, ``-ln P`` each; not normalised by the
    kernel) are float64 DEVICE tensors the host never reads, so a captured graph sees what they hold at replay.  A pixel whose
    ``log_prior`` is not finite is dead: no mass, ``-inf`` in ``post``, 0 in ``snr_map``, and nothing of its response or delays
    is used.  With ``K_{j,p} = sum_k C_{p,k} kappa_{k,j}(delay_{p,k})`` and ``HH_p = sum_k |C_{p,k}|^2 hh_k``:
    ``u_p = log_prior_p + logsumexp_j (ln I0(|K_{j,p}|) - HH_p / 2) - ln n_tau``, ``lnl_sky = logsumexp_p u_p``, ``pix_index``
    the smallest pixel of the largest ``u_p``, ``tau_index`` and ``snr`` as in the network call at that pixel, ``lnl_sky_mix``
    [B] the log-mean-exp of ``lnl_sky`` over the ``R / B`` latent samples; ``posterior=True`` adds ``post`` [R, P] = ``u_p -
    lnl_sky`` (the sky map) and ``post_mix`` [B, P], ``snr_map=True`` the best SNR of every pixel [R, P].
    ``include/npf_hip.h`` has the contract and the edge cases.  ``data``, ``weights``, ``taus``, ``n_valid``: as in
    :func:`waveform_loglike_network`.  ``freqs`` [T] is required, shared by all tasks, and must be finite.  ``want``: names out of
    ``LOGLIKE_SKY_NAMES``.  ``npf_waveform_loglike_sky``: one complex GEMM with M = R n_tau, N = P, K = D T on the double-precision
    matrix instruction -- the rotation by ``tau_j`` is done once per row, not once per pixel -- in three launches; inference only,
    no host sync, deterministic; the workspace is the one of :func:`waveform_match`.
    Out of scope: antenna patterns and delays from (ra, dec, psi, iota), which come from the caller's GW library; a sky grid per
    task; gradients; adaptive or hierarchical pixel refinement (distance jointly with the sky: :func:`waveform_loglike_sky_distance`)."""
    if isinstance(want, str) or not isinstance(want, (tuple, list)) or any(w not in LOGLIKE_SKY_NAMES for w in want):
        raise ValueError(f"want must be a tuple / list of names out of {LOGLIKE_SKY_NAMES}, got {want!r}")
    want = tuple(want)
    R, T, ld, B, D, P, wgt_rows, tau0, dtau, n_tau = check_loglike_sky_args(getattr(h, "shape", ()), data, response, delays, log_prior,
                                                                            weights, freqs, taus)
    if not want and not posterior and not snr_map:
        raise ValueError(f"want must name at least one of {LOGLIKE_SKY_NAMES} (or posterior=True / snr_map=True)")
    for t in (h, data, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    for t, what in ((response, "response"), (delays, "delays"), (log_prior, "log_prior")):
        if t is not None and (not t.is_cuda or t.device != h.device):
            raise ValueError(f"{what} must live on the device of h ({h.device}), got {t.device}: the kernel reads it there")
    h, data, freqs = h.detach().contiguous(), data.detach().contiguous(), freqs.detach().contiguous()
    response, delays = response.detach().contiguous(), delays.detach().contiguous()
    log_prior = log_prior.detach().contiguous() if log_prior is not None else None
    weights = weights.detach().contiguous() if weights is not None else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    lib = L.load()
    ws = _match_workspace(h.device, int(lib.npf_waveform_loglike_sky_workspace_bytes(R, D, T, P, n_tau)))
    out = {name: (torch.empty((B if name == "lnl_sky_mix" else R,), dtype=torch.int32 if name.endswith("index") else torch.float64,
                              device=h.device) if name in want else None) for name in LOGLIKE_SKY_NAMES}
    new = lambda rows: torch.empty((rows, P), dtype=torch.float64, device=h.device)  # noqa: E731
    post, post_mix = (new(R), new(B)) if posterior else (None, None)
    smap = new(R) if snr_map else None
    dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    L.check(lib.npf_waveform_loglike_sky(L.ptr(h), ld, L.ptr(data), L.ptr(weights), wgt_rows, L.ptr(freqs), 1,
                                         _iptr(nv) if nv is not None else None, dptr(response), dptr(delays), dptr(log_prior), R, B, D,
                                         T, P, tau0, dtau, n_tau, *(dptr(out[name]) for name in LOGLIKE_SKY_NAMES), dptr(post),
                                         dptr(smap), dptr(post_mix), ws.data_ptr(), L.stream_ptr()), "npf_waveform_loglike_sky")
    return WaveformLogLikeSky(*(out[name] for name in LOGLIKE_SKY_NAMES), post, post_mix, smap)


# ---- differentiable likelihoods (csrc/waveform_grad_kernels.hip) --------------
class WaveformLnl(NamedTuple):
    """What :func:`waveform_lnl` / :func:`waveform_lnl_network` return: the four likelihoods (float64, differentiable with respect to
    ``h``) and the grid index of the maximum (int32, not differentiable; 0 without ``taus``)."""
    lnl_marg: torch.Tensor     # [R]
    lnl_max: torch.Tensor      # [R]
    lnl_mix: torch.Tensor      # [B]
    lnl_max_mix: torch.Tensor  # [B]
    tau_index: torch.Tensor    # [R] int32


def _lnl_forward(net, h_eval, data, weights, freqs, nv, response, delays, geo):
    """The forward launches of ``npf_waveform_loglike_ex`` / ``npf_waveform_loglike_net_ex`` on prepared tensors -> (the five outputs,
    the float64 [R, 4 + 2 n] coefficients the backward launch starts from)."""
    lib = L.load()
    dev = h_eval.device
    dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    if net:
        R, T, ld, B, D, wgt_rows, freq_rows, tau0, dtau, n_tau = geo
        ws = _match_workspace(dev, int(lib.npf_waveform_loglike_net_workspace_bytes(R, D, n_tau)))
    else:
        R, T, ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau = geo
        ws = _match_workspace(dev, int(lib.npf_waveform_loglike_workspace_bytes(R, n_tau)))
    saved = torch.empty((R, int(lib.npf_waveform_loglike_saved_doubles(n_tau))), dtype=torch.float64, device=dev)
    marg, mx = (torch.empty((R,), dtype=torch.float64, device=dev) for _ in range(2))
    mix, mxm = (torch.empty((B,), dtype=torch.float64, device=dev) for _ in range(2))
    idx = torch.empty((R,), dtype=torch.int32, device=dev)
    head = (L.ptr(h_eval), ld, L.ptr(data), L.ptr(weights), wgt_rows, L.ptr(freqs), freq_rows, _iptr(nv) if nv is not None else None)
    outs = (None, None, None, mx.data_ptr(), marg.data_ptr(), idx.data_ptr(), None, None, mix.data_ptr(), mxm.data_ptr())
    if net:
        L.check(lib.npf_waveform_loglike_net_ex(*head, dptr(delays), dptr(response), R, B, D, T, tau0, dtau, n_tau, *outs, None, None,
                                                None, saved.data_ptr(), ws.data_ptr(), L.stream_ptr()), "npf_waveform_loglike_net_ex")
    else:
        L.check(lib.npf_waveform_loglike_ex(*head, R, B, T, tau0, dtau, n_tau, *outs, saved.data_ptr(), ws.data_ptr(), L.stream_ptr()),
                "npf_waveform_loglike_ex")
    return (marg, mx, mix, mxm, idx), saved


def _lnl_backward(net, tensors, geo, n_bcast, src_shape, grads):
    """One ``npf_waveform_loglike_bwd`` / ``npf_waveform_loglike_net_bwd`` launch -> the gradient of ``src``, written whole."""
    h_eval, data, weights, freqs, nv, response, delays, marg, mx, mix, mxm, idx, saved = tensors
    d_src = torch.empty(src_shape, dtype=torch.float32, device=h_eval.device)  # (written whole: no memset)
    if all(g is None for g in grads):
        return d_src.zero_()
    grads = [g.to(torch.float64).contiguous() if g is not None else None for g in grads]
    dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    head = (L.ptr(h_eval), geo[2], L.ptr(data), L.ptr(weights), geo[-5], L.ptr(freqs), geo[-4], _iptr(nv) if nv is not None else None)
    tail = (geo[-3], geo[-2], geo[-1], _iptr(idx), saved.data_ptr(), marg.data_ptr(), mx.data_ptr(), mix.data_ptr(), mxm.data_ptr(),
            *(dptr(g) for g in grads), n_bcast, L.ptr(d_src), src_shape[2], L.stream_ptr())
    lib = L.load()
    if net:
        L.check(lib.npf_waveform_loglike_net_bwd(*head, dptr(delays), dptr(response), geo[0], geo[3], geo[4], geo[1], *tail),
                "npf_waveform_loglike_net_bwd")
    else:
        L.check(lib.npf_waveform_loglike_bwd(*head, geo[0], geo[3], geo[1], *tail), "npf_waveform_loglike_bwd")
    return d_src


class _WaveformLnlFn(torch.autograd.Function):
    """The four likelihoods of the rows of ``h_eval`` under ``data`` (``npf_waveform_loglike_ex``, which keeps the row coefficients
    ``q_j`` in double) and their gradient with respect to ``src`` (one ``npf_waveform_loglike_bwd`` launch): ``src`` is ``h_eval``
    itself (``n_bcast`` = 1) or the [n_bcast * R, T, ld] samples whose mean over the ``n_bcast`` row blocks ``h_eval`` holds."""

    @staticmethod
    def forward(ctx, src, h_eval, data, weights, freqs, nv, geo, n_bcast):
        outs, saved = _lnl_forward(False, h_eval, data, weights, freqs, nv, None, None, geo)
        ctx.save_for_backward(h_eval, data, weights, freqs, nv, None, None, *outs, saved)
        ctx.cfg = (geo, n_bcast, tuple(src.shape))
        ctx.mark_non_differentiable(outs[4])
        ctx.set_materialize_grads(False)  # (an unused likelihood hands the launch a NULL, not a tensor of zeros)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_marg, d_max, d_mix, d_max_mix, _):
        geo, n_bcast, src_shape = ctx.cfg
        d_src = _lnl_backward(False, ctx.saved_tensors, geo, n_bcast, src_shape, (d_marg, d_max, d_mix, d_max_mix))
        return d_src, None, None, None, None, None, None, None


class _WaveformLnlNetworkFn(torch.autograd.Function):
    """:class:`_WaveformLnlFn` over the network sums (``npf_waveform_loglike_net_ex`` / ``npf_waveform_loglike_net_bwd``)."""

    @staticmethod
    def forward(ctx, src, h_eval, data, response, delays, weights, freqs, nv, geo, n_bcast):
        outs, saved = _lnl_forward(True, h_eval, data, weights, freqs, nv, response, delays, geo)
        ctx.save_for_backward(h_eval, data, weights, freqs, nv, response, delays, *outs, saved)
        ctx.cfg = (geo, n_bcast, tuple(src.shape))
        ctx.mark_non_differentiable(outs[4])
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_marg, d_max, d_mix, d_max_mix, _):
        geo, n_bcast, src_shape = ctx.cfg
        d_src = _lnl_backward(True, ctx.saved_tensors, geo, n_bcast, src_shape, (d_marg, d_max, d_mix, d_max_mix))
        return d_src, None, None, None, None, None, None, None, None, None


def _lnl_rows(who, h, n_bcast, mean):
    """The ``n_bcast`` / ``mean`` rules of :func:`waveform_mismatch` -> the tensor the likelihood is evaluated on (not yet detached)."""
    if isinstance(n_bcast, bool) or not isinstance(n_bcast, int) or n_bcast < 1:
        raise ValueError(f"n_bcast must be a host int >= 1, got {n_bcast!r}")
    if n_bcast > 1 and mean is None:
        raise ValueError(f"n_bcast > 1 evaluates {who} on `mean`, the mean of the n_bcast samples h holds: give it")
    h_shape = tuple(getattr(h, "shape", ()))
    if mean is not None:
        if len(h_shape) != 3 or h_shape[0] % n_bcast != 0 or h_shape[2] < 2:
            raise ValueError(f"h must have shape [n_bcast * R, T, >= 2] with n_bcast={n_bcast}, got {list(h_shape)}")
        if not isinstance(mean, torch.Tensor) or mean.dim() != 3 or tuple(mean.shape[:2]) != (h_shape[0] // n_bcast, h_shape[1]):
            raise ValueError(f"mean must have shape [R={h_shape[0] // n_bcast}, T={h_shape[1]}, >= 2], got "
                             f"{list(mean.shape) if isinstance(mean, torch.Tensor) else type(mean).__name__}")
    return h if mean is None else mean


def waveform_lnl(h: torch.Tensor, data: torch.Tensor, weights: Optional[torch.Tensor] = None, freqs: Optional[torch.Tensor] = None,
                 taus=None, n_valid: Optional[torch.Tensor] = None, n_bcast: int = 1, mean: Optional[torch.Tensor] = None) -> WaveformLnl:
    """``lnl_marg``, ``lnl_max`` [R], ``lnl_mix``, ``lnl_max_mix`` [B] and ``tau_index`` of :func:`waveform_loglike` (same arguments,
    same bits), the four likelihoods differentiable with respect to ``h``: the objective a waveform surrogate is trained on when it
    is to be used as the template in ``ln Lambda``.  The forward is the two launches of ``npf_waveform_loglike`` plus one that keeps
    the coefficients ``q_j = p_j I1 / I0 (x_j) conj(u_j)`` of every row in double; the backward is ONE ``npf_waveform_loglike_bwd``
    launch, the adjoint of the correlation launch, that forms the upstream scalars itself and writes the whole gradient of ``h``
    [.., T, ld] (``include/npf_hip.h`` has the formulae).  The gradient of ``lnl_marg`` / ``lnl_mix`` is exact, through the time
    marginal; that of ``lnl_max`` / ``lnl_max_mix`` is taken at the grid time the forward found (a tie: at the smaller index, a
    subgradient).  Entries 2 .. ld - 1 of a point, removed and padded points and rows with ``hh == 0`` get exact zeros.  No gradient
    with respect to ``data``, ``weights`` or ``freqs``: one of them with ``requires_grad`` is a ``ValueError``.  No double backward.
    ``n_bcast`` / ``mean``: as in :func:`waveform_mismatch`.  No host sync; the workspace is the one of :func:`waveform_match`, so
    inside a captured graph the call needs one earlier call at these sizes."""
    h_eval = _lnl_rows("the likelihood", h, n_bcast, mean)
    geo = check_loglike_args(getattr(h_eval, "shape", ()), data, weights, freqs, taus)
    for t, what in ((data, "data"), (weights, "weights"), (freqs, "freqs")):
        if t is not None and t.requires_grad:
            raise ValueError(f"waveform_lnl has no gradient with respect to {what}: detach it")
    for t in (h, mean, data, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    n_tau, B = geo[8], geo[3]
    h = h.contiguous()
    h_eval = h.detach() if mean is None else mean.detach().contiguous()
    weights = weights.detach().contiguous() if weights is not None else None
    freqs = freqs.detach().contiguous() if freqs is not None and n_tau > 0 else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    return WaveformLnl(*_WaveformLnlFn.apply(h, h_eval, data.detach().contiguous(), weights, freqs, nv, geo, n_bcast))


def waveform_lnl_network(h: torch.Tensor, data: torch.Tensor, response: torch.Tensor, delays: Optional[torch.Tensor] = None,
                         weights: Optional[torch.Tensor] = None, freqs: Optional[torch.Tensor] = None, taus=None,
                         n_valid: Optional[torch.Tensor] = None, n_bcast: int = 1, mean: Optional[torch.Tensor] = None) -> WaveformLnl:
    """:func:`waveform_lnl` of the coherent network likelihood: the values of :func:`waveform_loglike_network` (same arguments, same
    bits), differentiable with respect to ``h``.  One sum over the grid is shared by the detectors; the backward launch
    (``npf_waveform_loglike_net_bwd``) walks the detectors that are live at a point in ascending order.  No gradient with respect
    to ``data``, ``response``, ``delays``, ``weights`` or ``freqs`` (``requires_grad`` on one of them: ``ValueError``)."""
    h_eval = _lnl_rows("the likelihood", h, n_bcast, mean)
    geo = check_loglike_network_args(getattr(h_eval, "shape", ()), data, response, delays, weights, freqs, taus)
    for t, what in ((data, "data"), (response, "response"), (delays, "delays"), (weights, "weights"), (freqs, "freqs")):
        if t is not None and t.requires_grad:
            raise ValueError(f"waveform_lnl_network has no gradient with respect to {what}: detach it")
    for t in (h, mean, data, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    for t, what in ((response, "response"), (delays, "delays")):
        if t is not None and (not t.is_cuda or t.device != h.device):
            raise ValueError(f"{what} must live on the device of h ({h.device}), got {t.device}: the kernel reads it there")
    n_tau, B = geo[9], geo[3]
    h = h.contiguous()
    h_eval = h.detach() if mean is None else mean.detach().contiguous()
    delays = delays.detach().contiguous() if delays is not None else None
    weights = weights.detach().contiguous() if weights is not None else None
    freqs = freqs.detach().contiguous() if freqs is not None and (n_tau > 0 or delays is not None) else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    return WaveformLnl(*_WaveformLnlNetworkFn.apply(h, h_eval, data.detach().contiguous(), response.detach().contiguous(), delays,
                                                    weights, freqs, nv, geo, n_bcast))


# ---- distance-marginalised likelihood (csrc/waveform_dist_kernels.hip) --------------
DIST_SC = 16             # NPF_DIST_SC: scales per workgroup of the scale launch
DIST_MAX_SCALES = 4096   # NPF_DIST_MAX_SCALES
LOGLIKE_DIST_NAMES = ("lnl_dist", "scale_index", "scale_hat", "lnl_amp_max", "lnl_dist_mix")


class WaveformLogLikeDistance(NamedTuple):
    """What :func:`waveform_loglike_distance` / :func:`waveform_loglike_network_distance` return (float64 but the two indices); the
    entries that were not asked for are ``None``."""
    lnl_dist: Optional[torch.Tensor]      # [R] phase, time and amplitude scale marginalised
    scale_index: Optional[torch.Tensor]   # [R] int32: the smallest grid index of the largest evidence
    scale_hat: Optional[torch.Tensor]     # [R] x* / HH: the maximum-likelihood scale (not tied to the grid)
    lnl_amp_max: Optional[torch.Tensor]   # [R] x*^2 / (2 HH): the amplitude-maximised statistic
    lnl_dist_mix: Optional[torch.Tensor]  # [B] lnl_dist marginalised over the latent samples
    post: Optional[torch.Tensor]          # [R, n_a] log posterior mass of every scale
    post_mix: Optional[torch.Tensor]      # [B, n_a] the same, marginal over the latent samples
    base: object                          # the WaveformLogLike / WaveformLogLikeNetwork of the same call


def check_loglike_distance_args(h_shape, data, scales, log_prior, weights=None, freqs=None, taus=None, response=None, delays=None,
                                network=False):
    """The shapes and dtypes of a :func:`waveform_loglike_distance` call (``network=True``: of a
    :func:`waveform_loglike_network_distance` call) -> ``(geo, scale_rows, prior_rows, n_a)`` with ``geo`` what
    :func:`check_loglike_args` / :func:`check_loglike_network_args` return; ``ValueError`` for anything that does not fit.  ``scales``
    and ``log_prior``: float64 tensors [n_a] or [B, n_a] (each on its own), ``1 <= n_a <= DIST_MAX_SCALES``.  Reads no data."""
    geo = (check_loglike_network_args(h_shape, data, response, delays, weights, freqs, taus) if network
           else check_loglike_args(h_shape, data, weights, freqs, taus))
    B = geo[3]
    n_a = None
    rows = []
    for t, what in ((scales, "scales"), (log_prior, "log_prior")):
        if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.dtype != torch.float64:
            raise ValueError(f"{what} must be a float64 tensor of shape [n_a] or [B={B}, n_a], got "
                             f"{(list(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dim() == 2 and t.shape[0] != B:
            raise ValueError(f"{what} must have shape [n_a] or [B={B}, n_a], got {list(t.shape)}")
        if not 1 <= t.shape[-1] <= DIST_MAX_SCALES:
            raise ValueError(f"{what} holds {t.shape[-1]} scales: 1 <= n_a <= {DIST_MAX_SCALES}")
        if n_a is not None and t.shape[-1] != n_a:
            raise ValueError(f"scales holds {n_a} grid points, log_prior {t.shape[-1]}")
        n_a = t.shape[-1]
        rows.append(1 if t.dim() == 1 else B)
    return geo, rows[0], rows[1], n_a


def _distance_call(network, h, data, response, delays, scales, log_prior, weights, freqs, taus, n_valid, want, posterior):
    names = LOGLIKE_NET_NAMES if network else LOGLIKE_NAMES
    if isinstance(want, str) or not isinstance(want, (tuple, list)) or any(w not in names + LOGLIKE_DIST_NAMES for w in want):
        raise ValueError(f"want must be a tuple / list of names out of {names + LOGLIKE_DIST_NAMES}, got {want!r}")
    want = tuple(want)
    geo, scale_rows, prior_rows, n_a = check_loglike_distance_args(getattr(h, "shape", ()), data, scales, log_prior, weights, freqs, taus,
                                                                   response, delays, network)
    if network:
        R, T, ld, B, D, wgt_rows, freq_rows, tau0, dtau, n_tau = geo
    else:
        (R, T, ld, B, wgt_rows, freq_rows, tau0, dtau, n_tau), D = geo, 0
    if not want and not posterior:
        raise ValueError(f"want must name at least one of {names + LOGLIKE_DIST_NAMES} (or posterior=True)")
    for t in (h, data, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    for t, what in ((response, "response"), (delays, "delays"), (scales, "scales"), (log_prior, "log_prior")):
        if t is not None and (not t.is_cuda or t.device != h.device):
            raise ValueError(f"{what} must live on the device of h ({h.device}), got {t.device}: the kernel reads it there")
    h, data = h.detach().contiguous(), data.detach().contiguous()
    scales, log_prior = scales.detach().contiguous(), log_prior.detach().contiguous()
    response = response.detach().contiguous() if response is not None else None
    delays = delays.detach().contiguous() if delays is not None else None
    weights = weights.detach().contiguous() if weights is not None else None
    freqs = freqs.detach().contiguous() if freqs is not None and (n_tau > 0 or delays is not None) else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    lib = L.load()
    ws = _match_workspace(h.device, int(lib.npf_waveform_loglike_dist_workspace_bytes(R, D, n_tau, n_a)))

    def new(name):
        rows = B if name in _LOGLIKE_PER_TASK or name in ("dd_det", "lnl_dist_mix") else R
        return torch.empty((rows, D) if name in _LOGLIKE_NET_PER_DET else (rows,),
                           dtype=torch.int32 if name in ("tau_index", "scale_index") else torch.float64, device=h.device)

    out = {name: (new(name) if name in want else None) for name in names + LOGLIKE_DIST_NAMES}
    post = torch.empty((R, n_a), dtype=torch.float64, device=h.device) if posterior else None
    post_mix = torch.empty((B, n_a), dtype=torch.float64, device=h.device) if posterior else None
    dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    parent = [dptr(out[name]) for name in ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase")] + \
        [None, dptr(out["lnl_mix"]), dptr(out["lnl_max_mix"])]  # (no series: ``post`` is this call's grid output)
    tail = (dptr(scales), scale_rows, dptr(log_prior), prior_rows, n_a, *(dptr(out[name]) for name in LOGLIKE_DIST_NAMES), dptr(post),
            dptr(post_mix), ws.data_ptr(), L.stream_ptr())
    head = (L.ptr(h), ld, L.ptr(data), L.ptr(weights), wgt_rows, L.ptr(freqs), freq_rows, _iptr(nv) if nv is not None else None)
    if network:
        L.check(lib.npf_waveform_loglike_net_dist(*head, dptr(delays), dptr(response), R, B, D, T, tau0, dtau, n_tau, *parent,
                                                  dptr(out["hh_det"]), dptr(out["snr_det"]), dptr(out["dd_det"]), *tail),
                "npf_waveform_loglike_net_dist")
        base = WaveformLogLikeNetwork(*(out[name] for name in LOGLIKE_NET_NAMES), None)
    else:
        L.check(lib.npf_waveform_loglike_dist(*head, R, B, T, tau0, dtau, n_tau, *parent, *tail), "npf_waveform_loglike_dist")
        base = WaveformLogLike(*(out[name] for name in LOGLIKE_NAMES), None)
    return WaveformLogLikeDistance(*(out[name] for name in LOGLIKE_DIST_NAMES), post, post_mix, base)


def waveform_loglike_distance(h: torch.Tensor, data: torch.Tensor, scales: torch.Tensor, log_prior: torch.Tensor,
                              weights: Optional[torch.Tensor] = None, freqs: Optional[torch.Tensor] = None, taus=None,
                              n_valid: Optional[torch.Tensor] = None, want=LOGLIKE_NAMES + LOGLIKE_DIST_NAMES,
                              posterior: bool = False) -> WaveformLogLikeDistance:
    """The likelihood of :func:`waveform_loglike` marginalised over the amplitude scale of the template as well -- for a template
    ``h`` at a reference distance ``d_ref``, over the luminosity distance ``d = d_ref / a``.  ``scales`` (``a_i``) and ``log_prior``
    (``ln pi_i``, the log prior MASS of grid point ``i``, quadrature weight included; :func:`distance_prior` makes both from
    distances) are float64 DEVICE tensors [n_a] or [B, n_a], ``1 <= n_a <= DIST_MAX_SCALES``, taken as they are: the host reads
    neither, so a captured graph sees what they hold at replay.  A scale is live if ``0 < a_i < inf`` and ``ln pi_i`` is finite;
    nothing else of a dead scale is used.  With ``x_j = |kappa_j|``, ``x* = max_j x_j``, ``n = max(n_tau, 1)``:
    ``u_i = ln pi_i + ln I0(a_i x*) - a_i^2 hh / 2 + ln sum_j exp(ln I0(a_i x_j) - ln I0(a_i x*)) - ln n`` (``-inf`` for a dead scale)
    is the evidence of scale ``i``, marginal over phase and grid time; ``lnl_dist = logsumexp_i u_i`` (no live scale: ``-inf``),
    ``scale_index`` the smallest index of ``max_i u_i`` (no live scale: 0), ``scale_hat = x* / hh`` and ``lnl_amp_max = x*^2 / (2
    hh)`` the maximum-likelihood scale and statistic (0 for ``hh == 0``), ``lnl_dist_mix`` [B] the log-mean-exp of ``lnl_dist`` over
    the latent samples.  ``posterior=True`` adds ``post`` [R, n_a] ``= u_i - lnl_dist`` and ``post_mix`` [B, n_a], the log posterior
    mass of every scale per latent sample and marginal over them (``-inf`` at dead scales, everywhere when no scale is live).  The
    prior is not normalised by the kernel.  A row with ``hh == 0`` has ``Lambda = 1`` at every scale: ``post_i = ln pi_i -
    logsumexp ln pi``.  ``want``: names out of ``LOGLIKE_NAMES + LOGLIKE_DIST_NAMES``; the parent's come back in ``base``, from the
    parent's own kernels, bit-equal to a plain :func:`waveform_loglike` call (its finishing launch runs only if one is asked for).
    Launch 1 of the parent, then two ``npf_waveform_loglike_dist`` launches; double arithmetic, inference only, no host sync,
    deterministic; the workspace is the one of :func:`waveform_match`.  ``include/npf_hip.h`` has the contract."""
    return _distance_call(False, h, data, None, None, scales, log_prior, weights, freqs, taus, n_valid, want, posterior)


def waveform_loglike_network_distance(h: torch.Tensor, data: torch.Tensor, response: torch.Tensor, delays: Optional[torch.Tensor],
                                      scales: torch.Tensor, log_prior: torch.Tensor, weights: Optional[torch.Tensor] = None,
                                      freqs: Optional[torch.Tensor] = None, taus=None, n_valid: Optional[torch.Tensor] = None,
                                      want=LOGLIKE_NET_NAMES + LOGLIKE_DIST_NAMES, posterior: bool = False) -> WaveformLogLikeDistance:
    """:func:`waveform_loglike_distance` over the network sums of :func:`waveform_loglike_network` (``K_j``, ``HH`` in place of
    ``kappa_j``, ``hh``): one amplitude scale, one phase and one arrival time are shared by the detectors.  ``data``, ``response``,
    ``delays`` (``None``: zeros), ``weights``, ``freqs``, ``taus``, ``n_valid``: as in :func:`waveform_loglike_network`; ``scales``,
    ``log_prior``, ``posterior`` and the results: as in :func:`waveform_loglike_distance`; ``want``: names out of
    ``LOGLIKE_NET_NAMES + LOGLIKE_DIST_NAMES``."""
    return _distance_call(True, h, data, response, delays, scales, log_prior, weights, freqs, taus, n_valid, want, posterior)


def distance_prior(distances: torch.Tensor, d_ref: float, power: float = 2.0):
    """``(scales, log_prior)`` of :func:`waveform_loglike_distance` from a grid of luminosity distances: ``distances`` float64 [n_a]
    or [B, n_a], positive and increasing along the last axis (the units of ``d_ref``, the distance the template is predicted at).
    ``scales = d_ref / distances``; ``log_prior = ln(d^power x trapezoid width)`` -- the width of point ``i`` is half the distance
    between its neighbours, half the one interval at either end, 1 for a single point -- normalised to total mass 1 per row.
    ``power = 2``: uniform in volume.  Plain torch on the device of ``distances``; no host read."""
    if not isinstance(distances, torch.Tensor) or distances.dim() not in (1, 2) or distances.dtype != torch.float64 or \
            distances.shape[-1] < 1:
        raise ValueError("distances must be a float64 tensor of shape [n_a] or [B, n_a], got "
                         f"{(list(distances.shape), distances.dtype) if isinstance(distances, torch.Tensor) else type(distances).__name__}")
    d = distances.detach()
    if d.shape[-1] == 1:
        width = torch.ones_like(d)
    else:
        gap = d[..., 1:] - d[..., :-1]
        width = 0.5 * (torch.nn.functional.pad(gap, (1, 0)) + torch.nn.functional.pad(gap, (0, 1)))
    lp = float(power) * torch.log(d) + torch.log(width)
    return float(d_ref) / d, lp - torch.logsumexp(lp, -1, keepdim=True)


# ---- sky and distance marginalised jointly (csrc/waveform_sky_kernels.hip) --------------
SKYD_SC = 8  # NPF_SKYD_SC: scales per wavefront of the scale-marginal launch
LOGLIKE_SKY_DIST_NAMES = ("lnl_vol", "pix_index", "scale_index", "tau_index", "snr", "scale_hat", "lnl")


class WaveformLogLikeSkyDistance(NamedTuple):
    """What :func:`waveform_loglike_sky_distance` returns (float64 but the three indices); what was not asked for is ``None``."""
    lnl_vol: Optional[torch.Tensor]        # [R] phase, time, sky position and distance marginalised
    pix_index: Optional[torch.Tensor]      # [R] int32: the pixel of the largest distance-marginal evidence, the smallest index
    scale_index: Optional[torch.Tensor]    # [R] int32: the scale of the largest sky-marginal evidence, the smallest index
    tau_index: Optional[torch.Tensor]      # [R] int32: the grid time of the largest |K_j| at pixel pix_index
    snr: Optional[torch.Tensor]            # [R] max_j |K_j| / sqrt(HH) at that pixel
    scale_hat: Optional[torch.Tensor]      # [R] max_j |K_j| / HH at that pixel: the maximum-likelihood scale there
    lnl: Optional[torch.Tensor]            # [B] lnl_vol marginalised over the latent samples
    post_sky: Optional[torch.Tensor]       # [R, P] the sky map, distance marginalised (``posterior=True``)
    post_dist: Optional[torch.Tensor]      # [R, n_a] the distance posterior, sky marginalised (``posterior=True``)
    post_sky_mix: Optional[torch.Tensor]   # [B, P] (``posterior=True``)
    post_dist_mix: Optional[torch.Tensor]  # [B, n_a] (``posterior=True``)
    post_joint: Optional[torch.Tensor]     # [R, P, n_a] (``joint=True``)
    dist_mean: Optional[torch.Tensor]      # [R, P] E[d / d_ref | pixel] (``moments=True``)
    dist_std: Optional[torch.Tensor]       # [R, P] its spread (``moments=True``)


def check_loglike_sky_distance_args(h_shape, data, response, delays, scales, log_prior_scale, log_prior=None, weights=None, freqs=None,
                                    taus=None):
    """The shapes and dtypes of a :func:`waveform_loglike_sky_distance` call -> ``(geo, n_a)`` with ``geo`` what
    :func:`check_loglike_sky_args` returns, under its rules; ``scales`` and ``log_prior_scale``: float64 tensors [n_a], ``1 <= n_a <=
    DIST_MAX_SCALES`` -- one grid shared by the tasks, so [B, n_a] is refused.  ``ValueError`` for anything that does not fit.
    Reads no data."""
    geo = check_loglike_sky_args(h_shape, data, response, delays, log_prior, weights, freqs, taus)
    n_a = None
    for t, what in ((scales, "scales"), (log_prior_scale, "log_prior_scale")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.float64:
            raise ValueError(f"{what} must be a float64 tensor of shape [n_a] (one scale grid shared by the tasks), got "
                             f"{(list(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if not 1 <= t.shape[0] <= DIST_MAX_SCALES:
            raise ValueError(f"{what} holds {t.shape[0]} scales: 1 <= n_a <= {DIST_MAX_SCALES}")
        if n_a is not None and t.shape[0] != n_a:
            raise ValueError(f"scales holds {n_a} grid points, log_prior_scale {t.shape[0]}")
        n_a = t.shape[0]
    return geo, n_a


def waveform_loglike_sky_distance(h: torch.Tensor, data: torch.Tensor, response: torch.Tensor, delays: torch.Tensor,
                                  scales: torch.Tensor, log_prior_scale: torch.Tensor, log_prior: Optional[torch.Tensor] = None,
                                  weights: Optional[torch.Tensor] = None, freqs: Optional[torch.Tensor] = None, taus=None,
                                  n_valid: Optional[torch.Tensor] = None, want=LOGLIKE_SKY_DIST_NAMES, posterior: bool = False,
                                  joint: bool = False, moments: bool = False) -> WaveformLogLikeSkyDistance:
    """The likelihood of :func:`waveform_loglike_sky` marginalised over the amplitude scale of the template as well: sky and
    distance jointly, in one call.  ``h``, ``data``, ``response`` [P, D, 2], ``delays`` [P, D], ``log_prior`` [P] (pixels),
    ``weights``, ``freqs`` [T], ``taus``, ``n_valid``: as in :func:`waveform_loglike_sky`; ``scales`` [n_a] (``a_i``) and
    ``log_prior_scale`` [n_a] (``ln pi_i``; :func:`distance_prior` makes both) are float64 DEVICE tensors shared by the tasks, under
    the liveness rule of :func:`waveform_loglike_distance`; the host reads neither.  With ``x_{p,j} = |K_{j,p}|``:
    ``w_{p,i} = log_prior_p + ln pi_i + (logsumexp_j ln I0(a_i x_{p,j}) - ln n) - a_i^2 HH_p / 2`` (``-inf`` for a dead pixel or
    scale), ``lnl_vol = logsumexp_{p,i} w``, ``pix_index`` / ``scale_index`` the smallest index of the largest marginal evidence
    over the other axis, ``tau_index`` / ``snr`` as in the sky call at ``pix_index``, ``scale_hat = x* / HH`` there, ``lnl`` [B] the
    log-mean-exp of ``lnl_vol`` over the latent samples.  ``posterior=True`` adds ``post_sky`` [R, P], ``post_dist`` [R, n_a] and
    their mixtures [B, .]; ``joint=True`` ``post_joint`` [R, P, n_a]; ``moments=True`` ``dist_mean`` / ``dist_std`` [R, P], the
    conditional mean and spread of ``1 / a = d / d_ref`` at every pixel (0 at a dead pixel).  ``want``: names out of
    ``LOGLIKE_SKY_DIST_NAMES``.  ``npf_waveform_loglike_sky_dist``: four launches, double arithmetic, inference only, no host
    sync, deterministic; the workspace is the one of :func:`waveform_match`.  ``include/npf_hip.h`` has the contract.
    Out of scope: gradients; per-task or per-pixel scale grids; moments of the mixture over the latent samples; antenna patterns
    from angles; adaptive pixel refinement; continuous amplitude integration."""
    names = LOGLIKE_SKY_DIST_NAMES
    if isinstance(want, str) or not isinstance(want, (tuple, list)) or any(w not in names for w in want):
        raise ValueError(f"want must be a tuple / list of names out of {names}, got {want!r}")
    want = tuple(want)
    geo, n_a = check_loglike_sky_distance_args(getattr(h, "shape", ()), data, response, delays, scales, log_prior_scale, log_prior,
                                               weights, freqs, taus)
    R, T, ld, B, D, P, wgt_rows, tau0, dtau, n_tau = geo
    if not want and not posterior and not joint and not moments:
        raise ValueError(f"want must name at least one of {names} (or posterior=True / joint=True / moments=True)")
    for t, what in ((h, "h"), (data, "data"), (response, "response"), (delays, "delays"), (scales, "scales"),
                    (log_prior_scale, "log_prior_scale"), (log_prior, "log_prior"), (weights, "weights"), (freqs, "freqs")):
        if t is not None and t.requires_grad:
            raise ValueError(f"waveform_loglike_sky_distance is inference only: {what} requires grad; detach it")
    for t in (h, data, weights, freqs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")
    for t, what in ((response, "response"), (delays, "delays"), (log_prior, "log_prior"), (scales, "scales"),
                    (log_prior_scale, "log_prior_scale")):
        if t is not None and (not t.is_cuda or t.device != h.device):
            raise ValueError(f"{what} must live on the device of h ({h.device}), got {t.device}: the kernel reads it there")
    h, data, freqs = h.contiguous(), data.contiguous(), freqs.contiguous()
    response, delays = response.contiguous(), delays.contiguous()
    scales, log_prior_scale = scales.contiguous(), log_prior_scale.contiguous()
    log_prior = log_prior.contiguous() if log_prior is not None else None
    weights = weights.contiguous() if weights is not None else None
    nv = counts_i32(n_valid, B) if n_valid is not None else None
    lib = L.load()
    nbytes = int(lib.npf_waveform_loglike_sky_dist_workspace_bytes(R, D, T, P, n_tau, n_a))
    if nbytes < 0:
        raise ValueError(f"the workspace of {R} rows x {P} pixels x max({n_tau}, {n_a}) grid points does not fit a 64-bit byte count")
    ws = _match_workspace(h.device, nbytes)
    out = {name: (torch.empty((B if name == "lnl" else R,), dtype=torch.int32 if name.endswith("index") else torch.float64,
                              device=h.device) if name in want else None) for name in names}
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=h.device)  # noqa: E731
    post_sky, post_dist, sky_mix, dist_mix = (new(R, P), new(R, n_a), new(B, P), new(B, n_a)) if posterior else (None,) * 4
    post_joint = new(R, P, n_a) if joint else None
    mean, std = (new(R, P), new(R, P)) if moments else (None, None)
    dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    L.check(lib.npf_waveform_loglike_sky_dist(L.ptr(h), ld, L.ptr(data), L.ptr(weights), wgt_rows, L.ptr(freqs), 1,
                                              _iptr(nv) if nv is not None else None, dptr(response), dptr(delays), dptr(log_prior), R,
                                              B, D, T, P, tau0, dtau, n_tau, dptr(scales), dptr(log_prior_scale), n_a,
                                              *(dptr(out[name]) for name in names), dptr(post_sky), dptr(post_dist), dptr(post_joint),
                                              dptr(mean), dptr(std), dptr(sky_mix), dptr(dist_mix), ws.data_ptr(), L.stream_ptr()),
            "npf_waveform_loglike_sky_dist")
    return WaveformLogLikeSkyDistance(*(out[name] for name in names), post_sky, post_dist, sky_mix, dist_mix, post_joint, mean, std)


# ---- Monte-Carlo objectives over the latent samples -------------------------------------
MC_MEAN, MC_LOGMEANEXP, MC_SUMO = 0, 1, 2


class _McObjectiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_w, mode, inv_w, m):
        n_z, B = log_w.shape
        log_w = log_w.contiguous()
        out = torch.empty((B,), dtype=torch.float32, device=log_w.device)
        L.check(L.load().npf_mc_objective_fwd(L.ptr(log_w), n_z, B, mode, L.ptr(inv_w), m, L.ptr(out), L.stream_ptr()),
                "npf_mc_objective_fwd")
        ctx.save_for_backward(log_w, inv_w)
        ctx.cfg = (mode, m)
        return out

    @staticmethod
    def backward(ctx, d_out):
        log_w, inv_w = ctx.saved_tensors
        mode, m = ctx.cfg
        n_z, B = log_w.shape
        d = torch.empty_like(log_w)
        ws = torch.empty_like(log_w) if mode == MC_SUMO else None
        L.check(L.load().npf_mc_objective_bwd(L.ptr(log_w), n_z, B, mode, L.ptr(inv_w), m, L.ptr(d_out.contiguous()), L.ptr(d),
                                              L.ptr(ws), L.stream_ptr()), "npf_mc_objective_bwd")
        return d, None, None, None


def mc_objective(log_w: torch.Tensor, mode: int, inv_weights: Optional[torch.Tensor] = None, m: int = 0) -> torch.Tensor:
    """Per-task estimate [B] from the log weights ``log_w`` [n_z, B] of the latent samples
    (``npf_mc_objective_fwd``): their mean, log-mean-exp, or the SUMO estimate."""
    return _McObjectiveFn.apply(log_w, mode, inv_weights, m)


class _HeadsFn(torch.autograd.Function):
    """Heads as tasks and back on PT32 tensors (attention.py:505-527); the two directions are each
    other's adjoint."""

    @staticmethod
    def forward(ctx, x_pt, n_tasks, pts, F, n_heads, split):
        ctx.geom = (n_tasks, pts, F, n_heads, split)
        return _heads(x_pt, n_tasks, pts, F, n_heads, split)

    @staticmethod
    def backward(ctx, g):
        n_tasks, pts, F, n_heads, split = ctx.geom
        return _heads(g.contiguous(), n_tasks, pts, F, n_heads, not split), None, None, None, None, None


def _heads(x_pt, n_tasks, pts, F, n_heads, split):
    from .chain import pt_empty

    lib = L.load()
    x_pt = x_pt.contiguous()
    if split:
        out = pt_empty(n_heads * n_tasks, pts, F // n_heads, x_pt.device)
        L.check(lib.npf_split_heads(L.ptr(x_pt), n_tasks, pts, F, n_heads, L.ptr(out), L.stream_ptr()), "npf_split_heads")
    else:
        out = pt_empty(n_tasks, pts, F, x_pt.device)
        L.check(lib.npf_merge_heads(L.ptr(x_pt), n_tasks, pts, F, n_heads, L.ptr(out), L.stream_ptr()), "npf_merge_heads")
    return out


def split_heads(x_pt: torch.Tensor, n_tasks: int, pts: int, F: int, n_heads: int) -> torch.Tensor:
    """PT32 [n_tasks, pts, F] -> PT32 [n_heads * n_tasks, pts, F / n_heads] (task index h * n_tasks + b)."""
    return _HeadsFn.apply(x_pt, n_tasks, pts, F, n_heads, True)


def merge_heads(x_pt: torch.Tensor, n_tasks: int, pts: int, F: int, n_heads: int) -> torch.Tensor:
    """Inverse of :func:`split_heads`."""
    return _HeadsFn.apply(x_pt, n_tasks, pts, F, n_heads, False)


MHA_MAX_KEYS = {16: 256, 32: 128}  # head size -> keys the fused multihead attention kernel takes (csrc/mha_kernel.hip)
MHA_ENABLED = os.environ.get("NPF_NO_MHA", "0") != "1"  # NPF_NO_MHA=1: heads as extra tasks on the chain kernel (round 2)


class _MhaFn(torch.autograd.Function):
    """out[b, q, D h + :] = softmax_k(Q_h K_h^T / sqrt(D)) V_h on the PT32 tensors of the K / Q / V projections (``npf_mha_fwd`` /
    ``npf_mha_bwd``; MultiheadAttender.forward, npf/architectures/attention.py:505-527 with DotAttender :204-220 per head)."""

    @staticmethod
    def forward(ctx, q_pt, k_pt, v_pt, n_tasks, n_keys, n_queries, n_heads, head):
        F = n_heads * head
        q_pt, k_pt, v_pt = q_pt.contiguous(), k_pt.contiguous(), v_pt.contiguous()
        train = any(ctx.needs_input_grad[:3])
        # (zeros where the kernel leaves something unwritten: the features of a padded tile beyond F, the points beyond n_queries)
        whole = F % 32 == 0 and n_queries % 32 == 0
        out = (torch.empty if whole else torch.zeros)(CH.pt_shape(n_tasks, n_queries, F), dtype=torch.float32, device=q_pt.device)
        lse = torch.empty((n_tasks, n_heads, n_queries), dtype=torch.float32, device=q_pt.device) if train else None
        ev0 = CH.profile_begin()
        L.check(L.load().npf_mha_fwd(L.ptr(q_pt), L.ptr(k_pt), L.ptr(v_pt), n_tasks, n_heads, n_keys, n_queries, F, L.ptr(out),
                                     L.ptr(lse) if lse is not None else None, L.stream_ptr()), "npf_mha_fwd")
        CH.profile_end(ev0, "mha_fwd_kernel", 4 * n_tasks * n_queries * n_keys * F, 4 * F * n_tasks * (2 * n_queries + 2 * n_keys),
                       "multihead attention")
        ctx.geom = (n_tasks, n_keys, n_queries, n_heads, F)
        if train:
            ctx.save_for_backward(q_pt, k_pt, v_pt, out, lse)
        return out

    @staticmethod
    def backward(ctx, g):
        n_tasks, n_keys, n_queries, n_heads, F = ctx.geom
        q_pt, k_pt, v_pt, out, lse = ctx.saved_tensors
        g = g.contiguous()
        # (zeros where the kernel leaves something unwritten, as in the forward pass)
        mk = lambda t, n: (torch.empty_like if (F % 32 == 0 and n % 32 == 0) else torch.zeros_like)(t)  # noqa: E731
        dq, dk, dv = mk(q_pt, n_queries), mk(k_pt, n_keys), mk(v_pt, n_keys)
        ev0 = CH.profile_begin()
        L.check(L.load().npf_mha_bwd(L.ptr(q_pt), L.ptr(k_pt), L.ptr(v_pt), L.ptr(out), L.ptr(g), L.ptr(lse), n_tasks, n_heads,
                                     n_keys, n_queries, F, L.ptr(dq), L.ptr(dk), L.ptr(dv), L.stream_ptr()), "npf_mha_bwd")
        CH.profile_end(ev0, "mha_bwd_kernel", 14 * n_tasks * n_queries * n_keys * F, 4 * F * n_tasks * (4 * n_queries + 4 * n_keys),
                       "multihead attention backward")
        return dq, dk, dv, None, None, None, None, None


def mha_usable(kq_head: int, v_head: int, n_keys: int) -> bool:
    """Does the fused multihead attention kernel take this: fp32 mode, 16-feature heads and at most 256 keys, or 32-feature heads
    and at most 128."""
    from . import chain as CH

    return (MHA_ENABLED and CH.COMPUTE_DTYPE == "fp32" and kq_head == v_head and kq_head in MHA_MAX_KEYS
            and 0 < n_keys <= MHA_MAX_KEYS[kq_head])


def mha(q_pt: torch.Tensor, k_pt: torch.Tensor, v_pt: torch.Tensor, n_tasks: int, n_keys: int, n_queries: int,
        n_heads: int, head: int = 16) -> torch.Tensor:
    """PT32 [n_tasks, n_queries, head * n_heads]: per-head scaled-dot attention of the projected queries over the projected keys /
    values (``mha_usable``), no split / merge of heads in memory."""
    return _MhaFn.apply(q_pt, k_pt, v_pt, n_tasks, n_keys, n_queries, n_heads, head)


class _AddLayerNormFn(torch.autograd.Function):
    """LayerNorm(a + b) over the features on PT32 tensors (``npf_add_layernorm_fwd`` / ``_bwd``; the first LayerNorm of
    TransformerAttender.forward, npf/architectures/attention.py:566-575)."""

    @staticmethod
    def forward(ctx, a_pt, b_pt, gamma, beta, eps, n_tasks, pts, F):
        a_pt, b_pt = a_pt.contiguous(), b_pt.contiguous()
        tiles = tiles_of(pts)
        train = any(ctx.needs_input_grad[:4])
        y = (torch.zeros if pad32(F) != F else torch.empty)(CH.pt_shape(n_tasks, pts, F), dtype=torch.float32, device=a_pt.device)
        stats = torch.empty((n_tasks * tiles * 32, 2), dtype=torch.float32, device=a_pt.device) if train else None
        g, bt = gamma.detach().contiguous(), beta.detach().contiguous()
        ev0 = CH.profile_begin()
        L.check(L.load().npf_add_layernorm_fwd(L.ptr(a_pt), L.ptr(b_pt), L.ptr(g), L.ptr(bt), float(eps), n_tasks, pts, F, L.ptr(y),
                                               L.ptr(stats) if stats is not None else None, L.stream_ptr()), "npf_add_layernorm_fwd")
        CH.profile_end(ev0, "add_layernorm_fwd_kernel", 0, 12 * n_tasks * tiles * 32 * F, "LayerNorm(a + b)")
        ctx.geom = (n_tasks, pts, F, tiles)
        if train:
            ctx.save_for_backward(a_pt, b_pt, g, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        n_tasks, pts, F, tiles = ctx.geom
        a_pt, b_pt, g, stats = ctx.saved_tensors
        dy = dy.contiguous()
        dx = (torch.zeros if pad32(F) != F else torch.empty)(CH.pt_shape(n_tasks, pts, F), dtype=torch.float32, device=dy.device)
        partials = torch.empty((n_tasks * tiles, 2, F), dtype=torch.float32, device=dy.device)
        ev0 = CH.profile_begin()
        L.check(L.load().npf_add_layernorm_bwd(L.ptr(a_pt), L.ptr(b_pt), L.ptr(g), L.ptr(stats), L.ptr(dy), n_tasks, pts, F, L.ptr(dx),
                                               L.ptr(partials), L.stream_ptr()), "npf_add_layernorm_bwd")
        sums = partials.sum(0)
        CH.profile_end(ev0, "add_layernorm_bwd_kernel", 0, 16 * n_tasks * tiles * 32 * F, "LayerNorm(a + b) backward")
        return dx, dx, sums[0], sums[1], None, None, None, None


def add_layernorm_usable(F: int) -> bool:
    from . import chain as CH

    return MHA_ENABLED and CH.COMPUTE_DTYPE == "fp32" and F % 4 == 0 and F <= 256


def add_layernorm(a_pt: torch.Tensor, b_pt: torch.Tensor, ln: torch.nn.LayerNorm, n_tasks: int, pts: int) -> torch.Tensor:
    """PT32 LayerNorm(a + b) with the module's gamma / beta / eps (``add_layernorm_usable``)."""
    F = ln.normalized_shape[0]
    return _AddLayerNormFn.apply(a_pt, b_pt, ln.weight, ln.bias, ln.eps, n_tasks, pts, F)


# ---- padded contexts: per-task counts as device data (csrc/masked_kernels.hip) -------------------------------------------
MASKED_MAX_WIDTH = 256  # feature width of npf_masked_attn_fwd / _bwd


def counts_i32(n_valid: torch.Tensor, n_tasks: int, what: str = "n_valid") -> torch.Tensor:
    """The per-task counts as the contiguous device int32 [n_tasks] tensor the masked kernels read.  An int64 tensor is converted on
    the device; the values are never read by the host (the kernels clamp them to the rows the tensors hold)."""
    if not isinstance(n_valid, torch.Tensor):
        raise ValueError(f"{what} must be an integer device tensor of shape [{n_tasks}], got {type(n_valid).__name__}")
    if n_valid.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what} must be int32 or int64, got {n_valid.dtype}")
    if tuple(n_valid.shape) != (n_tasks,):
        raise ValueError(f"{what} must have shape [{n_tasks}] (one count per task), got {list(n_valid.shape)}")
    if not n_valid.is_cuda:
        raise ValueError(f"{what} must live on the device (its values are read by the kernels, never by the host)")
    return n_valid.to(torch.int32).contiguous()


def _query_counts(n_q_valid: Optional[torch.Tensor], n_tasks: int) -> Optional[torch.Tensor]:
    return None if n_q_valid is None else counts_i32(n_q_valid, n_tasks, "n_q_valid")


def _iptr(t: torch.Tensor) -> int:
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
    return t.data_ptr()


# ---- the refusals the wrappers below share (every wrapper keeps its own selection and order) -----------------------------------
def _check_width(d):
    if d % 4 != 0 or not 0 < d <= MASKED_MAX_WIDTH:
        raise NotImplementedError(f"masked attention takes feature widths that are multiples of 4 up to {MASKED_MAX_WIDTH}, got {d}")


def _check_sizes(**sizes):
    if any(v < 0 for v in sizes.values()):
        raise ValueError("negative size: " + ", ".join(f"{name}={v}" for name, v in sizes.items()))


def _check_replicates(n_tasks, n_src, src_name, reads):
    if n_src < 1 or n_tasks < 0 or n_tasks % n_src != 0:
        raise ValueError(f"n_tasks={n_tasks} must be a multiple of {src_name}={n_src} >= 1 (task j reads {reads} j % {src_name})")


def _check_pt32(what, t, n_tasks, pts, F, any_type=False):
    """Refuse ``t`` unless it is an fp32 PT32 tensor [n_tasks, pts, F].  ``any_type``: ``t`` may be no tensor at all (the
    differentiable wrappers, whose message then names its type)."""
    shape = tuple(pt_shape(n_tasks, pts, F))
    if any_type and not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be an fp32 PT32 tensor of shape {shape}, got {type(t).__name__}")
    if tuple(t.shape) != shape or t.dtype != torch.float32:
        got = (t.dtype, tuple(t.shape)) if any_type else f"{t.dtype} {tuple(t.shape)}"
        raise ValueError(f"{what} must be an fp32 PT32 tensor of shape {shape}, got {got}")


def _inference_operands(who, operands, F, w=None):
    """The PT32 operands ``(what, tensor, tasks, points)`` of an inference-only wrapper, detached and contiguous: refused where one
    of them (or the weights ``w``) requires grad, or is no fp32 PT32 tensor [tasks, points, F]."""
    if any(t.requires_grad for _, t, _, _ in operands) or (isinstance(w, torch.Tensor) and w.requires_grad):
        raise RuntimeError(f"{who} is inference only (no backward pass): detach the inputs")
    for what, t, n_tasks, pts in operands:
        _check_pt32(what, t, n_tasks, pts, F)
    return [t.detach().contiguous() for _, t, _, _ in operands]


def _attend_no_grad(entry, q_pt, keys, n_q_valid, sizes, n_queries, d, scale):
    """PT32 [sizes[0], n_queries, d] from a forward-only entry point ``entry(q, *keys, n_q_valid, *sizes, n_queries, d, scale, out,
    stream)``: ``keys`` are the entry's key-side pointers, ``sizes`` its task and key sizes, both in its own order."""
    out = torch.empty(pt_shape(sizes[0], n_queries, d), dtype=torch.float32, device=q_pt.device)  # (written whole)
    L.check(getattr(L.load(), entry)(L.ptr(q_pt), *keys, _iptr(n_q_valid) if n_q_valid is not None else None, *sizes, n_queries, d,
                                     float(scale), L.ptr(out), L.stream_ptr()), entry)
    return out


# PROFILE names and notes of _MaskedAttnFn, without / with key weights
_MASKED_FWD_PROFILE = (("masked_attn_fwd_kernel", "masked attention (flops at full counts)"),
                       ("masked_attn_fwd_weighted_kernel", "key-weighted attention (flops at full counts)"))
_MASKED_BWD_PROFILE = (("masked_attn_bwd_kernels", "masked attention backward (flops at full counts)"),
                       ("masked_attn_bwd_weighted_kernels", "key-weighted attention backward (flops at full counts)"))


class _MaskedAttnFn(torch.autograd.Function):
    """out[b, q] = softmax over the first n_valid[b] keys of scale <Q[b, q], K[b, k]> times V on PT32 tensors (``npf_masked_attn_fwd`` /
    ``_bwd``; DotAttender.forward, npf/architectures/attention.py:129-164,204-220, of the batch cut per task).  With ``w`` (else
    None) a weight per (task, key): ``p_k ~ w_k exp(s_k)`` (``npf_masked_attn_fwd_weighted`` / ``_fwd_weighted_ex`` at one
    replicate, ``npf_masked_attn_bwd_weighted``), differentiable in q, k, v and w."""

    @staticmethod
    def forward(ctx, q_pt, k_pt, v_pt, w, n_valid, n_tasks, n_keys, n_queries, d, scale, n_q_valid):
        q_pt, k_pt, v_pt = q_pt.contiguous(), k_pt.contiguous(), v_pt.contiguous()
        train = any(ctx.needs_input_grad[:4])
        out = torch.empty(pt_shape(n_tasks, n_queries, d), dtype=torch.float32, device=q_pt.device)  # (written whole)
        lse = torch.empty((n_tasks, n_queries), dtype=torch.float32, device=q_pt.device) if train else None
        ev0 = CH.profile_begin()
        if w is None:
            # (n_q_valid: padded queries as well, the instances that skip them)
            name, q_counts = ("npf_masked_attn_fwd", ()) if n_q_valid is None else ("npf_masked_attn_fwd_nq", (_iptr(n_q_valid),))
            L.check(getattr(L.load(), name)(L.ptr(q_pt), L.ptr(k_pt), L.ptr(v_pt), _iptr(n_valid), *q_counts, n_tasks, n_keys, n_queries,
                                            d, float(scale), L.ptr(out), L.ptr(lse) if lse is not None else None, L.stream_ptr()), name)
        else:
            w = w.contiguous()
            name, keep = ("npf_masked_attn_fwd_weighted", ()) if lse is None else ("npf_masked_attn_fwd_weighted_ex", (L.ptr(lse),))
            L.check(getattr(L.load(), name)(L.ptr(q_pt), L.ptr(k_pt), L.ptr(v_pt), L.ptr(w), _iptr(n_valid),
                                            _iptr(n_q_valid) if n_q_valid is not None else None, n_tasks, n_tasks, n_keys, n_queries, d,
                                            float(scale), L.ptr(out), *keep, L.stream_ptr()), name)
        CH.profile_end(ev0, _MASKED_FWD_PROFILE[w is not None][0], 4 * n_tasks * n_queries * n_keys * d,
                       4 * pad32(d) * n_tasks * (2 * n_queries + 2 * n_keys), _MASKED_FWD_PROFILE[w is not None][1])
        ctx.geom = (n_tasks, n_keys, n_queries, d, float(scale))
        if train:
            ctx.save_for_backward(q_pt, k_pt, v_pt, w, n_valid, out, lse, n_q_valid)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        n_tasks, n_keys, n_queries, d, scale = ctx.geom
        q_pt, k_pt, v_pt, w, n_valid, out, lse, n_q_valid = ctx.saved_tensors
        g = g.contiguous()
        dq, dk, dv = torch.empty_like(q_pt), torch.empty_like(k_pt), torch.empty_like(v_pt)  # (written whole)
        dw = None if w is None else torch.empty_like(w)
        ev0 = CH.profile_begin()
        if w is None:
            name, q_counts = ("npf_masked_attn_bwd", ()) if n_q_valid is None else ("npf_masked_attn_bwd_nq", (_iptr(n_q_valid),))
            L.check(getattr(L.load(), name)(L.ptr(q_pt), L.ptr(k_pt), L.ptr(v_pt), _iptr(n_valid), *q_counts, L.ptr(out), L.ptr(g),
                                            L.ptr(lse), n_tasks, n_keys, n_queries, d, scale, L.ptr(dq), L.ptr(dk), L.ptr(dv),
                                            L.stream_ptr()), name)
        else:
            L.check(L.load().npf_masked_attn_bwd_weighted(L.ptr(q_pt), L.ptr(k_pt), L.ptr(v_pt), L.ptr(w), _iptr(n_valid),
                                                          _iptr(n_q_valid) if n_q_valid is not None else None, L.ptr(out), L.ptr(g),
                                                          L.ptr(lse), n_tasks, n_keys, n_queries, d, scale, L.ptr(dq), L.ptr(dk),
                                                          L.ptr(dv), L.ptr(dw), L.stream_ptr()), "npf_masked_attn_bwd_weighted")
        CH.profile_end(ev0, _MASKED_BWD_PROFILE[w is not None][0], 16 * n_tasks * n_queries * n_keys * d,
                       4 * pad32(d) * n_tasks * (6 * n_queries + 4 * n_keys), _MASKED_BWD_PROFILE[w is not None][1])
        return dq, dk, dv, dw, None, None, None, None, None, None, None


def masked_attention(q_pt: torch.Tensor, k_pt: torch.Tensor, v_pt: torch.Tensor, n_valid: torch.Tensor, n_tasks: int, n_keys: int,
                     n_queries: int, d: int, scale: float, n_q_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PT32 [n_tasks, n_queries, d]: scaled-dot attention of every task's queries over the first ``n_valid[task]`` of its ``n_keys``
    keys / values (zeros where a task has none).  ``n_valid``: device int32 / int64 [n_tasks], read by the kernel only -- no host
    sync, so the call can be captured in a graph and replayed with new counts.  ``d`` % 4 == 0, ``d`` <= 256, any ``n_keys``.
    ``n_q_valid``: the same for the queries (padded targets): the rows of the result at and beyond ``n_q_valid[task]`` are zeros, the
    queries there are never read and get a zero gradient, and the kernels skip them (``npf_masked_attn_fwd_nq`` / ``_bwd_nq``); the
    rows below the counts are bit-identical to the call without it."""
    _check_width(d)
    n_q_valid = _query_counts(n_q_valid, n_tasks)
    return _MaskedAttnFn.apply(q_pt, k_pt, v_pt, None, counts_i32(n_valid, n_tasks), n_tasks, n_keys, n_queries, d, scale, n_q_valid)


def masked_attention_prefix(q_pt: torch.Tensor, k_pre: torch.Tensor, v_pre: torch.Tensor, n_prefix: torch.Tensor, k_tail: torch.Tensor,
                            v_tail: torch.Tensor, n_tail: torch.Tensor, n_tasks: int, n_prefix_tasks: int, c_pad: int, m_tail: int,
                            n_queries: int, d: int, scale: float, n_q_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PT32 [n_tasks, n_queries, d]: scaled-dot attention of task ``j`` over the first ``n_prefix[j % n_prefix_tasks]`` rows of PREFIX
    task ``j % n_prefix_tasks`` (``k_pre`` / ``v_pre``: PT32 [n_prefix_tasks, c_pad, d], shared by the ``n_tasks / n_prefix_tasks``
    tasks that map to it) followed by the first ``n_tail[j]`` rows of its own tail (``k_tail`` / ``v_tail``: PT32 [n_tasks, m_tail, d]);
    zeros where both counts are 0 (``npf_masked_attn_fwd_prefix``).  Counts and ``n_q_valid`` as in :func:`masked_attention`: device
    int32 / int64, read by the kernel only.  Inference only -- there is no backward pass, and a call in which an input requires grad
    is refused."""
    _check_width(d)
    _check_replicates(n_tasks, n_prefix_tasks, "n_prefix_tasks", "prefix")
    _check_sizes(c_pad=c_pad, m_tail=m_tail, n_queries=n_queries)
    q_pt, k_pre, v_pre, k_tail, v_tail = _inference_operands("masked_attention_prefix", (
        ("q_pt", q_pt, n_tasks, n_queries), ("k_pre", k_pre, n_prefix_tasks, c_pad), ("v_pre", v_pre, n_prefix_tasks, c_pad),
        ("k_tail", k_tail, n_tasks, m_tail), ("v_tail", v_tail, n_tasks, m_tail)), d)
    n_prefix, n_tail = counts_i32(n_prefix, n_prefix_tasks, "n_prefix"), counts_i32(n_tail, n_tasks, "n_tail")
    n_q_valid = _query_counts(n_q_valid, n_tasks)
    keys = (L.ptr(k_pre), L.ptr(v_pre), _iptr(n_prefix), L.ptr(k_tail), L.ptr(v_tail), _iptr(n_tail))
    return _attend_no_grad("npf_masked_attn_fwd_prefix", q_pt, keys, n_q_valid, (n_tasks, n_prefix_tasks, c_pad, m_tail), n_queries, d, scale)


def masked_attention_loo(q_pt: torch.Tensor, k_pt: torch.Tensor, v_pt: torch.Tensor, n_valid: torch.Tensor, n_tasks: int, n_keys: int,
                         n_queries: int, d: int, scale: float, n_q_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PT32 [n_tasks, n_queries, d]: :func:`masked_attention` in which query row ``t`` of a task does not see key row ``t`` of that
    task (``npf_masked_attn_fwd_loo``) -- with the encoded context points as queries and keys, every context point attends over the
    OTHER points of its task.  Exact zeros where no other key is left (a task with one point or none) and beyond ``n_q_valid``;
    ``v_pt`` row ``t`` has no influence on row ``t`` of the result.  Counts as in :func:`masked_attention`: device int32 / int64, read
    by the kernel only.  Inference only -- there is no backward pass, and a call in which an input requires grad is refused."""
    _check_width(d)
    _check_sizes(n_tasks=n_tasks, n_keys=n_keys, n_queries=n_queries)
    q_pt, k_pt, v_pt = _inference_operands("masked_attention_loo", (
        ("q_pt", q_pt, n_tasks, n_queries), ("k_pt", k_pt, n_tasks, n_keys), ("v_pt", v_pt, n_tasks, n_keys)), d)
    n_valid = counts_i32(n_valid, n_tasks)
    n_q_valid = _query_counts(n_q_valid, n_tasks)
    keys = (L.ptr(k_pt), L.ptr(v_pt), _iptr(n_valid))
    return _attend_no_grad("npf_masked_attn_fwd_loo", q_pt, keys, n_q_valid, (n_tasks, n_keys), n_queries, d, scale)


def loo_mean(R_pt: torch.Tensor, n_valid: torch.Tensor, n_tasks: int, pts: int, F: int) -> torch.Tensor:
    """PT32 [n_tasks, pts, F]: row ``i < n_valid[task]`` is the mean over the task's first ``n_valid[task]`` points WITHOUT point ``i``,
    ``(sum - R[i]) / (n - 1)`` (``npf_loo_mean``: the sum is taken in the launch and held in double, as are the subtraction and the
    division, with one rounding to fp32 -- a row that dwarfs the others of its task still gets their mean, and with two points the rows
    swap bit for bit; the bits are not those of :func:`masked_mean`); zeros beyond the count and where a task has one point or none.  Counts as in :func:`masked_attention`.  Inference only: a call in which the input
    requires grad is refused."""
    if n_tasks < 0 or pts < 1 or F < 1:
        raise ValueError(f"loo_mean needs n_tasks >= 0, pts >= 1 and F >= 1, got {n_tasks}, {pts}, {F}")
    if R_pt.requires_grad:
        raise RuntimeError("loo_mean is inference only (no backward pass): detach the input")
    _check_pt32("R_pt", R_pt, n_tasks, pts, F)
    n_valid = counts_i32(n_valid, n_tasks)
    R_pt = R_pt.detach().contiguous()
    out = torch.empty_like(R_pt)  # (written whole)
    L.check(L.load().npf_loo_mean(L.ptr(R_pt), _iptr(n_valid), n_tasks, pts, pad32(F), L.ptr(out), L.stream_ptr()), "npf_loo_mean")
    return out


def key_weights(w: torch.Tensor, n_tasks: int, n_keys: int, what: str = "w", detach: bool = True) -> torch.Tensor:
    """The per-(task, key) weights as the contiguous device fp32 [n_tasks, n_keys] tensor the weighted kernels read: any float
    tensor with ``n_tasks * n_keys`` elements whose leading dims multiply to ``n_tasks``; a contiguous fp32 tensor is used as given
    (a view, no copy), so weights overwritten in place are seen by a replayed graph.  The values are never read by the host.
    ``detach=False`` (the training route): the tensor stays in the autograd graph."""
    if not isinstance(w, torch.Tensor) or not w.is_floating_point():
        raise ValueError(f"{what} must be a float device tensor [..., {n_keys}] with {n_tasks} rows, got "
                         f"{w.dtype if isinstance(w, torch.Tensor) else type(w).__name__}")
    if w.dim() < 2 or w.shape[-1] != n_keys or w.numel() != n_tasks * n_keys:
        raise ValueError(f"{what} must hold one weight per (task, key): {n_tasks} rows of {n_keys}, got {list(w.shape)}")
    if not w.is_cuda:
        raise ValueError(f"{what} must live on the device (its values are read by the kernels, never by the host)")
    return (w.detach() if detach else w).to(torch.float32).contiguous().view(n_tasks, n_keys)


def masked_attention_weighted(q_pt: torch.Tensor, k_pt: torch.Tensor, v_pt: torch.Tensor, w: torch.Tensor, n_valid: torch.Tensor,
                              n_tasks: int, n_ctx_tasks: int, n_keys: int, n_queries: int, d: int, scale: float,
                              n_q_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PT32 [n_tasks, n_queries, d]: ``n_tasks = S * n_ctx_tasks`` replicates of :func:`masked_attention` over ONE stored copy of the
    context (``npf_masked_attn_fwd_weighted``).  Task ``j`` reads the queries, keys, values and counts of context task
    ``j % n_ctx_tasks`` (``q_pt`` PT32 [n_ctx_tasks, n_queries, d], ``k_pt`` / ``v_pt`` PT32 [n_ctx_tasks, n_keys, d], ``n_valid`` /
    ``n_q_valid`` [n_ctx_tasks]) and row ``j`` of ``w`` (float [n_tasks, n_keys], or [S, n_ctx_tasks, n_keys]): softmax probabilities
    ``p_k ~ w_k exp(s_k)`` over the keys below the count with ``0 < w_k < inf`` -- a weight that is 0, negative, NaN or Inf removes
    the key, an integer weight is "the point appears w times".  Exact zeros where no key is admissible and beyond ``n_q_valid``; with
    every weight 1.0 and one replicate the bits of :func:`masked_attention`.  Counts and weights are read by the kernel only.
    Inference only -- there is no backward pass, and a call in which an input requires grad is refused."""
    _check_width(d)
    _check_replicates(n_tasks, n_ctx_tasks, "n_ctx_tasks", "context task")
    _check_sizes(n_keys=n_keys, n_queries=n_queries)
    q_pt, k_pt, v_pt = _inference_operands("masked_attention_weighted", (
        ("q_pt", q_pt, n_ctx_tasks, n_queries), ("k_pt", k_pt, n_ctx_tasks, n_keys), ("v_pt", v_pt, n_ctx_tasks, n_keys)), d, w)
    w = key_weights(w, n_tasks, n_keys)
    n_valid = counts_i32(n_valid, n_ctx_tasks)
    n_q_valid = _query_counts(n_q_valid, n_ctx_tasks)
    keys = (L.ptr(k_pt), L.ptr(v_pt), L.ptr(w), _iptr(n_valid))
    return _attend_no_grad("npf_masked_attn_fwd_weighted", q_pt, keys, n_q_valid, (n_tasks, n_ctx_tasks, n_keys), n_queries, d, scale)


def weighted_mean(R_pt: torch.Tensor, w: torch.Tensor, n_valid: torch.Tensor, n_tasks: int, n_ctx_tasks: int, pts: int,
                  F: int) -> torch.Tensor:
    """Row-major [n_tasks, pad32(F)]: row ``j`` is the ``w[j]``-weighted mean over the admissible points (below
    ``n_valid[j % n_ctx_tasks]``, ``0 < w < inf``) of context task ``j % n_ctx_tasks`` of the PT32 tensor ``R_pt``
    [n_ctx_tasks, pts, F], zeros where the admissible weights sum to 0 (``npf_weighted_mean``: sums and division in double, one
    rounding, fixed order).  ``w``: float [n_tasks, pts] (or [S, n_ctx_tasks, pts]).  Counts and weights as in
    :func:`masked_attention_weighted`.  Inference only: a call in which an input requires grad is refused."""
    _check_replicates(n_tasks, n_ctx_tasks, "n_ctx_tasks", "context task")
    if pts < 1 or F < 1:
        raise ValueError(f"weighted_mean needs pts >= 1 and F >= 1, got {pts}, {F}")
    (R_pt,) = _inference_operands("weighted_mean", (("R_pt", R_pt, n_ctx_tasks, pts),), F, w)
    w = key_weights(w, n_tasks, pts)
    n_valid = counts_i32(n_valid, n_ctx_tasks)
    out = torch.empty((n_tasks, pad32(F)), dtype=torch.float32, device=R_pt.device)  # (written whole)
    L.check(L.load().npf_weighted_mean(L.ptr(R_pt), L.ptr(w), _iptr(n_valid), n_tasks, n_ctx_tasks, pts, pad32(F), L.ptr(out),
                                       L.stream_ptr()), "npf_weighted_mean")
    return out


# ---- training through key weights (npf_masked_attn_fwd_weighted_ex / _bwd_weighted, npf_weighted_mean_bwd) -------------------
def key_weighted_attention(q_pt: torch.Tensor, k_pt: torch.Tensor, v_pt: torch.Tensor, w: torch.Tensor, n_valid: torch.Tensor,
                           n_tasks: int, n_keys: int, n_queries: int, d: int, scale: float,
                           n_q_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PT32 [n_tasks, n_queries, d]: :func:`masked_attention` with a weight per (task, key) -- softmax probabilities
    ``p_k ~ w_k exp(scale <q, k>)`` over the keys below ``n_valid[task]`` with ``0 < w_k < inf`` -- DIFFERENTIABLE in ``q_pt``,
    ``k_pt``, ``v_pt`` and ``w`` (float [n_tasks, n_keys]): the training route of :func:`masked_attention_weighted` at one replicate.
    An integer weight is "the point appears w times"; with every weight 1.0 the forward bits are those of :func:`masked_attention`.
    ``d w_k = (sum_q dA_qk) / w_k`` (``include/npf_hip.h`` has the formulae); a key that is not admissible -- beyond the count, or
    with a weight that is 0, negative, NaN or Inf -- never meets a multiply and gets exact zeros in ``d k``, ``d v`` and ``d w``:
    a removed point is removed, there is no one-sided derivative at ``w = 0``.  The log-sum-exp is kept only when a gradient is
    needed (``npf_masked_attn_fwd_weighted_ex``, else ``npf_masked_attn_fwd_weighted``); the backward pass is one
    ``npf_masked_attn_bwd_weighted`` call (two launches, no atomics, every output written whole).  Counts, ``n_q_valid`` and weights
    are read by the kernels only: no host sync, and a captured call sees weights overwritten in place.  No double backward."""
    _check_width(d)
    _check_sizes(n_tasks=n_tasks, n_keys=n_keys, n_queries=n_queries)
    for what, t, pts in (("q_pt", q_pt, n_queries), ("k_pt", k_pt, n_keys), ("v_pt", v_pt, n_keys)):
        _check_pt32(what, t, n_tasks, pts, d, any_type=True)
    w = key_weights(w, n_tasks, n_keys, detach=False)
    n_valid = counts_i32(n_valid, n_tasks)
    return _MaskedAttnFn.apply(q_pt, k_pt, v_pt, w, n_valid, n_tasks, n_keys, n_queries, d, scale, _query_counts(n_q_valid, n_tasks))


class _KeyWeightedMeanFn(torch.autograd.Function):
    """The ``w``-weighted mean over the admissible points of every task (``npf_weighted_mean`` at one replicate /
    ``npf_weighted_mean_bwd``), differentiable in the points and in ``w``."""

    @staticmethod
    def forward(ctx, R_pt, w, n_valid, n_tasks, pts, F):
        Fp = pad32(F)
        R_pt, w = R_pt.contiguous(), w.contiguous()
        out = torch.empty((n_tasks, Fp), dtype=torch.float32, device=R_pt.device)  # (written whole)
        L.check(L.load().npf_weighted_mean(L.ptr(R_pt), L.ptr(w), _iptr(n_valid), n_tasks, n_tasks, pts, Fp, L.ptr(out), L.stream_ptr()),
                "npf_weighted_mean")
        ctx.geo = (n_tasks, pts, Fp)
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(R_pt, w, n_valid, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        n_tasks, pts, Fp = ctx.geo
        R_pt, w, n_valid, out = ctx.saved_tensors
        dR, dw = torch.empty_like(R_pt), torch.empty_like(w)  # (written whole)
        L.check(L.load().npf_weighted_mean_bwd(L.ptr(R_pt), L.ptr(w), _iptr(n_valid), L.ptr(out), L.ptr(g.contiguous()), n_tasks, pts, Fp,
                                               L.ptr(dR), L.ptr(dw), L.stream_ptr()), "npf_weighted_mean_bwd")
        return dR, dw, None, None, None, None


def key_weighted_mean(R_pt: torch.Tensor, w: torch.Tensor, n_valid: torch.Tensor, n_tasks: int, pts: int, F: int) -> torch.Tensor:
    """Row-major [n_tasks, pad32(F)]: row ``j`` is the ``w[j]``-weighted mean over the admissible points (below ``n_valid[j]``,
    ``0 < w < inf``) of task ``j`` of the PT32 tensor ``R_pt`` [n_tasks, pts, F], zeros where the admissible weights sum to 0 --
    :func:`weighted_mean` at one replicate (``npf_weighted_mean``, the same bits), DIFFERENTIABLE in ``R_pt`` and in ``w`` (float
    [n_tasks, pts]): ``d r_k = (w_k / W) d out`` and ``d w_k = <d out, r_k - out> / W`` with ``W`` the sum of the admissible weights
    (``npf_weighted_mean_bwd``: double arithmetic, one rounding, fixed order); exact zeros for the points that are not admissible
    and for a task with ``W = 0`` -- no one-sided derivative at ``w = 0``.  With integer weights: the mean over the context with
    its rows repeated.  Counts and weights are read by the kernels only.  No double backward."""
    if n_tasks < 0 or pts < 1 or F < 1:
        raise ValueError(f"key_weighted_mean needs n_tasks >= 0, pts >= 1 and F >= 1, got {n_tasks}, {pts}, {F}")
    _check_pt32("R_pt", R_pt, n_tasks, pts, F, any_type=True)
    w = key_weights(w, n_tasks, pts, detach=False)
    return _KeyWeightedMeanFn.apply(R_pt, w, counts_i32(n_valid, n_tasks), n_tasks, pts, F)


def masked_mean(R_pt: torch.Tensor, n_valid: torch.Tensor, n_tasks: int, pts: int, F: int) -> torch.Tensor:
    """Mean over the first ``n_valid[task]`` points of a PT32 tensor -> row-major [n_tasks, pad32(F)] (zeros where a task has none):
    ``torch.mean(R, dim=1)`` (npf/neuralproc/np.py:95, attnnp.py:181) of the batch cut per task; counts as in :func:`masked_attention`."""
    return _MeanFn.apply(R_pt, counts_i32(n_valid, n_tasks), n_tasks, pts, F)


# ---- growing contexts: rows appended at per-task offsets that are device data (csrc/append_kernels.hip) ----------------------
def append_points(pairs, n_valid: torch.Tensor, n_new: Optional[torch.Tensor], n_tasks: int, n_rows: int, capacity: int) -> None:
    """Append ``n_rows`` new rows per task to padded PT32 tensors, in place (``npf_append_points``: one launch for the rows of all
    pairs, one behind it for the counts).  ``pairs``: up to three ``(src, dst, F)`` with ``src`` PT32 [n_tasks, n_rows, F] and ``dst``
    PT32 [n_tasks, capacity, F]; row ``j < clamp(n_new[b], 0, n_rows)`` of ``src`` (``n_new`` None: every row) becomes row
    ``n_valid[b] + j`` of ``dst``, rows that would land at or beyond ``capacity`` are dropped, no other row is written, and then
    ``n_valid[b] <- min(n_valid[b] + n_new[b], capacity)``.  ``n_valid`` (updated in place) / ``n_new``: contiguous device int32
    [n_tasks] tensors, read by the kernels only.  No host read, no allocation, no autograd: the call can sit in a captured graph."""
    pairs = list(pairs)
    if not 1 <= len(pairs) <= L.NPF_APPEND_MAX_PAIRS:
        raise ValueError(f"append_points takes 1 to {L.NPF_APPEND_MAX_PAIRS} (src, dst, F) pairs, got {len(pairs)}")
    if n_rows < 0 or capacity < 1:
        raise ValueError(f"append_points needs n_rows >= 0 and capacity >= 1, got {n_rows} and {capacity}")
    for what, t in (("n_valid", n_valid), ("n_new", n_new)):
        if t is None and what == "n_new":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (n_tasks,) or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous int32 tensor of shape [{n_tasks}]")
        if not t.is_cuda:
            raise ValueError(f"{what} must live on the device (its values are read by the kernels, never by the host)")
    arr = (L.NpfAppendPair * len(pairs))()
    for i, (src, dst, F) in enumerate(pairs):
        if tuple(src.shape) != pt_shape(n_tasks, n_rows, F) or tuple(dst.shape) != pt_shape(n_tasks, capacity, F):
            raise ValueError(f"pair {i}: expected PT32 tensors of shapes {pt_shape(n_tasks, n_rows, F)} -> {pt_shape(n_tasks, capacity, F)}, "
                             f"got {tuple(src.shape)} -> {tuple(dst.shape)}")
        if src.device != n_valid.device or dst.device != n_valid.device:
            raise ValueError(f"pair {i} and the counts live on different devices")
        arr[i].src, arr[i].dst, arr[i].F = L.ptr(src), L.ptr(dst), pad32(F)
    L.check(L.load().npf_append_points(arr, len(pairs), _iptr(n_valid), _iptr(n_new) if n_new is not None else None, n_tasks, n_rows,
                                       capacity, L.stream_ptr()), "npf_append_points")
