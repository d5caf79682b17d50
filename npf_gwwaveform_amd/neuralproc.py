"""Members of the neural-process family with the reference's class interface and HIP
execution: ``CNP``, ``LNP``, ``AttnCNP``, ``AttnLNP``.

Mirrors (constructor kwargs, method names, return values, ``state_dict`` keys):
  * ``NeuralProcessFamily`` / ``LatentNeuralProcessFamily``   npf/neuralproc/base.py:23-575
  * ``CNP`` / ``LNP``                                         npf/neuralproc/np.py:19-163
  * ``AttnCNP`` / ``AttnLNP``                                 npf/neuralproc/attnnp.py:27-202

``forward`` runs the whole path as a handful of fused chain-kernel launches on PT32 tensors
(x-encoder, xy-encoder, [attention + merge +] decoder, Gaussian head); the stage methods
(``encode_globally``, ``trgt_dependent_representation``, ``latent_path``, ``decode``) keep
the reference's row-major signatures and run the same kernels stage by stage.
The reference's building blocks are supported (MLP x-encoder incl. ``is_res``, sum- or concatenating-merge
MLP xy-encoder / decoder, ``x_transf_dim`` != ``r_dim``, ``attention`` = scaledot / multihead / transformer);
anything else raises ``NotImplementedError`` -- there is no fallback path.
"""
from __future__ import annotations

import abc
import math
from functools import partial
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
from torch.distributions import Independent, Normal

from . import functional as FN
from .architectures import (MLP, DotAttender, KeyWeights, LeaveOneOut, MergeFlatInputs, MultiheadAttender, PrefixTail, SelfAttention,
                            TrainKeyWeights, as_key_rule, get_attender, merge_flat_input)
from .chain import Chain, PTensor, pad32, pt_shape

__all__ = ["NeuralProcessFamily", "LatentNeuralProcessFamily", "CNP", "LNP", "AttnCNP", "AttnLNP",
           "MultivariateNormalDiag", "HeadDistribution", "Conditioned", "Prediction", "Score", "Match", "BankMatch", "LogLike", "NetworkLogLike", "SkyLogLike", "SkyDistanceLogLike", "DistanceLogLike",
           "NetworkDistanceLogLike", "Reweighted", "bootstrap_weights",
           "kfold_weights"]


def MultivariateNormalDiag(loc, scale_diag):
    """npf/utils/helpers.py:125-129 (argument validation off: it would sync the stream)."""
    if loc.dim() < 1:
        raise ValueError("loc must be at least one-dimensional.")
    return Independent(Normal(loc, scale_diag, validate_args=False), 1)


class Prediction(NamedTuple):
    """Summary of the predictive distribution p(y | context) at the queried points (:meth:`HeadDistribution.summary`): for a
    latent model the equal-weight mixture over the latent samples of the Gaussians the head makes, else that one Gaussian."""
    mean: torch.Tensor       # [B, T, y_dim]
    std: torch.Tensor        # [B, T, y_dim]
    quantiles: torch.Tensor  # [len(probs), B, T, y_dim]
    probs: Tuple[float, ...]


class Score(NamedTuple):
    """Scores of observed values under the predictive distribution (:meth:`HeadDistribution.score`), per target point and output
    dimension; the entries that were not asked for are ``None``."""
    log_density: Optional[torch.Tensor]  # [B, T, y_dim] log of the predictive density at y
    pit: Optional[torch.Tensor]          # [B, T, y_dim] predictive CDF at y (probability integral transform)
    crps: Optional[torch.Tensor]         # [B, T, y_dim] continuous ranked probability score


class Match(NamedTuple):
    """Match of predicted waveforms against reference waveforms (:meth:`HeadDistribution.match`), one entry per (latent sample,
    task): [n_z, B] for ``of="samples"``, [1, B] for ``of="mean"``; the entries that were not computed are ``None``."""
    overlap: torch.Tensor              # Re <h, g> / sqrt(<h, h> <g, g>): no phase or time maximisation
    match: torch.Tensor                # max over the constant phase and the time-shift grid
    mismatch: torch.Tensor             # 1 - match, formed in double
    tau: Optional[torch.Tensor]        # float64: the grid time that attains the match (``taus`` given)
    tau_index: Optional[torch.Tensor]  # int32: its index on the grid, the smallest one (``taus`` given)
    phase: torch.Tensor                # arg of the correlation there
    corr: Optional[torch.Tensor]       # [.., B, max(n_tau, 1), 2] normalised correlation over the whole grid (``corr=True``)


class BankMatch(NamedTuple):
    """Match of every predicted waveform against every template of a bank (:meth:`HeadDistribution.match_bank`): [n_z, B, G] per
    (latent sample, task, template) and [n_z, B] per (latent sample, task); ``n_z = 1`` for ``of="mean"``."""
    match: torch.Tensor                # [n_z, B, G] max over the constant phase and the time-shift grid
    mismatch: torch.Tensor             # [n_z, B, G] 1 - match, formed in double
    tau: Optional[torch.Tensor]        # [n_z, B, G] float64: the grid time that attains the match (``taus`` given)
    tau_index: Optional[torch.Tensor]  # [n_z, B, G] int32: its index on the grid, the smallest one (``taus`` given)
    phase: torch.Tensor                # [n_z, B, G] arg of the correlation there
    best_index: torch.Tensor           # [n_z, B] int32: the template of the largest match, the smallest index
    best_match: torch.Tensor           # [n_z, B] the match there
    dot: Optional[torch.Tensor]        # [n_z, B, G, 2] float64: the unrounded correlation at the maximum (``dot=True``)


class LogLike(NamedTuple):
    """Matched-filter likelihood of complex data under the predicted waveforms (:meth:`HeadDistribution.loglike`), float64 (but
    ``tau_index``).  Per (latent sample, task): [n_z, B] for ``of="samples"``, [1, B] for ``of="mean"``; per task: [B]."""
    optimal_snr: torch.Tensor          # sqrt(<h|h>)
    snr: torch.Tensor                  # max over phase and grid times of <d|h> / sqrt(<h|h>)
    lnl_max: torch.Tensor              # ln Lambda maximised over the phase and the grid times
    lnl_marg: torch.Tensor             # ln Lambda marginalised over the phase and the grid times (uniform priors)
    phase: torch.Tensor                # arg of <d|h> at the maximum
    tau: Optional[torch.Tensor]        # the grid time of the maximum (``taus`` given)
    tau_index: Optional[torch.Tensor]  # int32: its index on the grid, the smallest one (``taus`` given)
    lnl: torch.Tensor                  # [B] lnl_marg marginalised over the latent samples: log-mean-exp
    lnl_max_mix: torch.Tensor          # [B] the same of lnl_max
    dd: torch.Tensor                   # [B] <d|d>; ln L = ln Lambda - dd / 2 + const
    series: Optional[torch.Tensor]     # [.., B, max(n_tau, 1), 2] = (L_j, SNR_j) over the whole grid (``series=True``)


class NetworkLogLike(NamedTuple):
    """Coherent matched-filter likelihood of the data of a detector network under the predicted waveforms
    (:meth:`HeadDistribution.loglike_network`), float64 (but ``tau_index``).  The fields of :class:`LogLike`, taken over the network
    sums, plus the detectors' own shares.  Per (latent sample, task): [n_z, B] for ``of="samples"``, [1, B] for ``of="mean"``; per
    task: [B]; per detector: a last axis of ``D``."""
    optimal_snr: torch.Tensor          # sqrt(sum_k |C_k|^2 <h|h>_k): the optimal network SNR
    snr: torch.Tensor                  # max over phase and grid times of |sum_k C_k <d_k|h>_k| / optimal_snr
    lnl_max: torch.Tensor              # ln Lambda maximised over the shared phase and the grid times
    lnl_marg: torch.Tensor             # ln Lambda marginalised over the shared phase and the grid times (uniform priors)
    phase: torch.Tensor                # arg of the network sum at the maximum
    tau: Optional[torch.Tensor]        # the (geocentric) grid time of the maximum (``taus`` given)
    tau_index: Optional[torch.Tensor]  # int32: its index on the grid, the smallest one (``taus`` given)
    lnl: torch.Tensor                  # [B] lnl_marg marginalised over the latent samples: log-mean-exp
    lnl_max_mix: torch.Tensor          # [B] the same of lnl_max
    dd: torch.Tensor                   # [B] sum_k <d_k|d_k>; ln L = ln Lambda - dd / 2 + const
    series: Optional[torch.Tensor]     # [.., B, max(n_tau, 1), 2] = (L_j, SNR_j) over the whole grid (``series=True``)
    snr_det: torch.Tensor              # [.., B, D] |<d_k|h>_k| / sqrt(<h|h>_k) at the network's grid time
    optimal_snr_det: torch.Tensor      # [.., B, D] |C_k| sqrt(<h|h>_k)
    dd_det: torch.Tensor               # [B, D] <d_k|d_k>


class SkyLogLike(NamedTuple):
    """Sky-grid network likelihood (:meth:`HeadDistribution.loglike_sky`), float64 (but the indices).  Per (latent sample, task):
    [n_z, B] for ``of="samples"``, [1, B] for ``of="mean"``; per task: [B]; per pixel: a last axis of ``P``."""
    lnl: torch.Tensor                  # [B] lnl_sky marginalised over the latent samples: log-mean-exp
    lnl_sky: torch.Tensor              # ln Lambda marginalised over the shared phase, the grid times and the sky pixels (prior as given)
    pix_index: torch.Tensor            # int32: the pixel of the largest evidence, the smallest index
    tau_index: Optional[torch.Tensor]  # int32: the grid time of the largest |K_j| at that pixel, the smallest one (``taus`` given)
    tau: Optional[torch.Tensor]        # that grid time (``taus`` given)
    snr: torch.Tensor                  # the network SNR at that pixel and grid time
    post: Optional[torch.Tensor]       # [.., B, P] log posterior mass of every pixel: the sky map (``posterior=True``)
    post_mix: Optional[torch.Tensor]   # [B, P] the same with the latent samples marginalised (``posterior=True``)
    snr_map: Optional[torch.Tensor]    # [.., B, P] the best network SNR of every pixel (``snr_map=True``)


class SkyDistanceLogLike(NamedTuple):
    """Sky and distance marginalised jointly (:meth:`HeadDistribution.loglike_sky_distance`), float64 (but the indices).  Per (latent
    sample, task): [n_z, B] for ``of="samples"``, [1, B] for ``of="mean"``; per task: [B]; per pixel / scale: a last axis of ``P`` /
    ``n_a``."""
    lnl: torch.Tensor                      # [B] lnl_vol marginalised over the latent samples: log-mean-exp
    lnl_vol: torch.Tensor                  # ln Lambda marginalised over phase, grid times, sky pixels and amplitude scales
    pix_index: torch.Tensor                # int32: the pixel of the largest distance-marginal evidence, the smallest index
    scale_index: torch.Tensor              # int32: the scale of the largest sky-marginal evidence, the smallest index
    scale_map: torch.Tensor                # ``scales`` gathered there
    tau_index: Optional[torch.Tensor]      # int32: the grid time of the largest |K_j| at pixel pix_index (``taus`` given)
    tau: Optional[torch.Tensor]            # that grid time (``taus`` given)
    snr: torch.Tensor                      # the network SNR at that pixel and grid time
    scale_hat: torch.Tensor                # the maximum-likelihood scale at that pixel; distance d_ref / scale_hat
    post_sky: Optional[torch.Tensor]       # [.., B, P] the sky map with the distance marginalised (``posterior=True``)
    post_dist: Optional[torch.Tensor]      # [.., B, n_a] the distance posterior with the sky marginalised (``posterior=True``)
    post_sky_mix: Optional[torch.Tensor]   # [B, P] the sky map with the latent samples marginalised too (``posterior=True``)
    post_dist_mix: Optional[torch.Tensor]  # [B, n_a] the same of the distance posterior (``posterior=True``)
    post_joint: Optional[torch.Tensor]     # [.., B, P, n_a] the joint log posterior mass (``joint=True``)
    dist_mean: Optional[torch.Tensor]      # [.., B, P] E[d / d_ref | pixel]: with dist_std the volume map (``moments=True``)
    dist_std: Optional[torch.Tensor]       # [.., B, P] the spread of d / d_ref at the pixel (``moments=True``)


class DistanceLogLike(NamedTuple):
    """Distance-marginalised likelihood (:meth:`HeadDistribution.loglike_distance`), float64 (but the indices).  Per (latent sample,
    task): [n_z, B] for ``of="samples"``, [1, B] for ``of="mean"``; per task: [B]; per scale: a last axis of ``n_a``."""
    lnl: torch.Tensor                  # [B] lnl_dist marginalised over the latent samples: log-mean-exp
    lnl_dist: torch.Tensor             # ln Lambda marginalised over phase, grid times and the amplitude scale (prior mass as given)
    scale_hat: torch.Tensor            # <d|h> / <h|h> at the maximum: the maximum-likelihood scale; distance d_ref / scale_hat
    lnl_amp_max: torch.Tensor          # snr^2 / 2: ln Lambda maximised over phase, grid times and amplitude
    scale_index: torch.Tensor          # int32: the grid scale of the largest evidence, the smallest index
    scale_map: torch.Tensor            # ``scales`` gathered there
    post: Optional[torch.Tensor]       # [.., B, n_a] log posterior mass of every scale (``posterior=True``)
    post_mix: Optional[torch.Tensor]   # [B, n_a] the same with the latent samples marginalised (``posterior=True``)
    base: LogLike                      # :meth:`HeadDistribution.loglike` of the same call (no series)


class NetworkDistanceLogLike(NamedTuple):
    """:class:`DistanceLogLike` over the network sums (:meth:`HeadDistribution.loglike_network_distance`); ``base`` is the
    :class:`NetworkLogLike` of the same call."""
    lnl: torch.Tensor
    lnl_dist: torch.Tensor
    scale_hat: torch.Tensor
    lnl_amp_max: torch.Tensor
    scale_index: torch.Tensor
    scale_map: torch.Tensor
    post: Optional[torch.Tensor]
    post_mix: Optional[torch.Tensor]
    base: NetworkLogLike


class Lnl(NamedTuple):
    """The differentiable likelihoods of :meth:`HeadDistribution.lnl` / :meth:`HeadDistribution.lnl_network`, float64, with the bits
    of :meth:`HeadDistribution.loglike` / :meth:`HeadDistribution.loglike_network`."""
    lnl: torch.Tensor          # [B] lnl_marg marginalised over the latent samples: log-mean-exp
    lnl_marg: torch.Tensor     # [n_z, B] ([1, B] for ``of="mean"``) phase and grid times marginalised
    lnl_max: torch.Tensor      # [n_z, B] ([1, B]) phase and grid times maximised
    lnl_max_mix: torch.Tensor  # [B] the log-mean-exp of lnl_max


def _as_loglike(m, taus, lead) -> LogLike:
    """A ``functional.WaveformLogLike`` (every name but ``tau_index`` without ``taus``) with its per-row entries shaped ``lead``."""
    tau = m.tau_index.double().mul_(float(taus[1])).add_(float(taus[0])).view(lead) if taus is not None else None
    return LogLike(m.hh.sqrt().view(lead), m.snr.view(lead), m.lnl_max.view(lead), m.lnl_marg.view(lead), m.phase.view(lead),
                   tau, m.tau_index.view(lead) if taus is not None else None, m.lnl_mix, m.lnl_max_mix, m.dd,
                   m.series.view(*lead, *m.series.shape[1:]) if m.series is not None else None)


def _as_network_loglike(m, taus, lead, response) -> NetworkLogLike:
    """The same of a ``functional.WaveformLogLikeNetwork``."""
    D = response.shape[1]
    tau = m.tau_index.double().mul_(float(taus[1])).add_(float(taus[0])).view(lead) if taus is not None else None
    c_abs = torch.hypot(response[..., 0], response[..., 1]).detach()  # [B, D] |C_k|, on the device
    return NetworkLogLike(m.hh.sqrt().view(lead), m.snr.view(lead), m.lnl_max.view(lead), m.lnl_marg.view(lead),
                          m.phase.view(lead), tau, m.tau_index.view(lead) if taus is not None else None, m.lnl_mix,
                          m.lnl_max_mix, m.dd, m.series.view(*lead, *m.series.shape[1:]) if m.series is not None else None,
                          m.snr_det.view(*lead, D), m.hh_det.sqrt().view(*lead, D) * c_abs, m.dd_det)


class HeadDistribution(Independent):
    """``MultivariateNormalDiag(loc, scale)`` of the decoder's raw output (base.py:350-367) -- an
    ``Independent(Normal(loc, scale), 1)`` with batch shape [n_z, B, T] and event shape [y_dim] -- evaluated lazily:
    ``loc`` / ``scale`` are only materialised ([n_z, B, T, y_dim] each, one ``npf_gauss_head_fwd`` launch) when
    ``base_dist`` (or anything that needs it: ``mean``, ``log_prob``, ``sample`` ...) is first touched.  The
    training and evaluation objectives never do: :meth:`sum_log_prob` is a loss-only launch that writes one float
    per (z-sample, task).

    ``n_trgt`` (device int32 [B]): the targets are padded, task ``b`` owns its first ``n_trgt[b]`` rows.  ``sum_log_prob`` and the
    homoskedastic pooling then cover those rows only, and the rows beyond have ``loc = 0``, ``scale = 1``."""

    def __init__(self, suff, y_dim, homoskedastic, n_z, B, T, n_trgt=None):
        torch.distributions.Distribution.__init__(self, torch.Size((n_z, B, T)), torch.Size((y_dim,)), validate_args=False)
        self.reinterpreted_batch_ndims = 1
        self._suff, self._y_dim, self._homosk, self._n_trgt = suff, y_dim, homoskedastic, n_trgt
        self._base = None
        self._slp = None  # (targets, [n_z, B] sum of log-probabilities) of the last sum_log_prob call

    @property
    def base_dist(self):
        if self._base is None:
            n_z, B, T = self.batch_shape
            loc, scale, _ = FN.gauss_head(self._suff, None, self._y_dim, self._homosk, n_valid=self._n_trgt)
            self._base = Normal(loc.view(n_z, B, T, self._y_dim), scale.view(n_z, B, T, self._y_dim), validate_args=False)
        return self._base

    def sum_log_prob(self, Y_trgt):
        """sum_t log p(y_t) -> [n_z, B] (npf/losses.py:18-24), fused with the head in one loss-only launch."""
        if self._slp is None or self._slp[0] is not Y_trgt:
            n_z, B, _ = self.batch_shape
            _, _, slp = FN.gauss_head(self._suff, Y_trgt.contiguous(), self._y_dim, self._homosk, want_dist=False,
                                      n_valid=self._n_trgt)
            self._slp = (Y_trgt, slp.view(n_z, B))
        return self._slp[1]

    def summary(self, probs=(0.025, 0.5, 0.975)) -> Prediction:
        """Mean, standard deviation and the ``probs``-quantiles of the predictive distribution per target point and output
        dimension, marginal over the latent samples (the equal-weight mixture of the ``n_z`` Gaussians): one
        ``npf_mixture_summary`` launch on the raw decoder output.  ``loc`` / ``scale`` are not materialised (``base_dist`` is left
        alone) and nothing of size [n_z, B, T, y_dim] is written.  Inference only: no gradient flows through the result.  ``probs``:
        a host sequence of probabilities strictly inside (0, 1); padded rows (``n_trgt``) get mean 0, std 1 and the standard-normal
        quantiles."""
        probs = FN.check_probs(probs)
        n_z = self.batch_shape[0]
        mean, std, quant = FN.mixture_summary(self._suff, n_z, self._y_dim, self._homosk, probs=probs, n_valid=self._n_trgt)
        return Prediction(mean, std, quant, probs)


    def score(self, Y_trgt, want=FN.SCORE_NAMES) -> Score:
        """How well the predictive distribution fits the observed ``Y_trgt`` [B, T, y_dim] -> :class:`Score` of [B, T, y_dim]
        tensors: ``log_density`` (log of the predictive density at y), ``pit`` (the predictive CDF at y: uniform on (0, 1) for a
        calibrated model) and ``crps`` (the continuous ranked probability score, in the units of y, smaller is better).  The
        predictive distribution is the one :meth:`summary` describes: marginal over the latent samples (the equal-weight mixture
        of the ``n_z`` Gaussians) and marginal per output dimension -- for CNP / AttnCNP, whose predictive is a product of
        independent Gaussians, the joint log density of a point is the sum of ``log_density`` over the last axis.  One
        ``npf_mixture_score`` launch on the raw decoder output: ``loc`` / ``scale`` are not materialised (``base_dist`` is left
        alone), nothing of size [n_z, B, T, y_dim] is written, no host sync; inference only.  ``want``: the names to compute, the
        others come back ``None`` and cost nothing.  With padded targets (``n_trgt``; for :meth:`NeuralProcessFamily.loo` the
        context counts) the rows beyond a task's count hold ``log_density = 0`` and ``crps = 0``, so a sum over T needs no mask,
        and ``pit = 0.5``: a PIT histogram must be masked by the counts."""
        want = FN.check_want(want)
        n_z = self.batch_shape[0]
        return Score(*FN.mixture_score(self._suff, Y_trgt, n_z, self._y_dim, self._homosk, n_valid=self._n_trgt, want=want))

    def match(self, Y_ref, weights=None, freqs=None, taus=None, of="samples", corr=False) -> Match:
        """The match of the predicted waveforms against the reference waveforms ``Y_ref`` [B, T, 2] -> :class:`Match`, for a model
        whose two outputs are (amplitude, phase): the waveform is ``A e^{i phi}``, the match the noise-weighted complex inner product
        ``sum_t w A A' exp(i (phi - phi'))`` normalised by both norms and maximised over a constant phase and, with ``taus =
        (tau0, dtau, n_tau)``, over the time shifts ``tau0 + j dtau`` (``freqs``, the physical frequency of every point in Hz, then
        carries the shift: ``2 pi f tau``); ``mismatch = 1 - match`` is formed in double, so values of 1e-8 survive.  ``weights``: the
        caller's ``4 df / S_n(f)`` per point ([T] or [B, T]; ``None``: ones); a point whose weight is not in (0, inf) is removed.
        ``of="samples"``: one entry per latent sample and task, [n_z, B] -- for a latent model the distribution of the mismatch over
        the sampled functions -- computed on the raw decoder output (``loc`` / ``scale`` are not materialised, ``base_dist`` is
        left alone).  ``of="mean"``: the match of the mixture-mean amplitude and phase (one moments-only ``npf_mixture_summary``
        launch), [1, B].  Padded targets (``n_trgt``) are left out.  ``corr=True`` adds the normalised correlation over the whole
        grid.  Two ``npf_waveform_match`` launches in double arithmetic; inference only, no host sync, so a ``query`` and its
        ``match`` can be captured in one graph (call once at the sizes before capturing: the workspace is allocated then)."""
        if self._y_dim != 2:
            raise ValueError(f"match needs a model whose two outputs are (amplitude, phase): y_dim == 2, got {self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_match_args((rows, T, ld), Y_ref, weights, freqs, taus)
        if of == "samples":
            h = self._suff.detach().reshape(rows, T, ld)
        else:
            h = FN.mixture_summary(self._suff, n_z, self._y_dim, self._homosk, n_valid=self._n_trgt)[0]
        want = ("overlap", "match", "mismatch", "phase") + (("tau_index",) if taus is not None else ())
        m = FN.waveform_match(h, Y_ref, weights, freqs, taus, n_valid=self._n_trgt, want=want, corr=corr)
        lead = (rows // B, B)
        tau = m.tau_index.double().mul_(float(taus[1])).add_(float(taus[0])).view(lead) if taus is not None else None
        return Match(m.overlap.view(lead), m.match.view(lead), m.mismatch.view(lead), tau,
                     m.tau_index.view(lead) if taus is not None else None, m.phase.view(lead),
                     m.corr.view(*lead, *m.corr.shape[1:]) if corr else None)

    def match_bank(self, bank, weights=None, freqs=None, taus=None, of="samples", dot=False) -> BankMatch:
        """The match of every predicted waveform against every template of ``bank`` [G, T, 2] = (amplitude, phase) -> :class:`BankMatch`:
        which template a prediction falls on (``best_index``, ``best_match``) and, with the predictions themselves as the bank,
        which waveforms are distinguishable at all.  Every match is maximised over the constant phase and the grid ``taus = (tau0,
        dtau, n_tau)`` as in :meth:`match`, in the same double arithmetic.  The bank is shared by the tasks, so ``weights`` and
        ``freqs`` are [T] and the prediction must sit on one grid: padded targets (``n_trgt``) are refused.  ``of="samples"``: on the
        raw decoder output, [n_z, B, G] (``base_dist`` is left alone); ``of="mean"``: the mixture-mean amplitude and phase, [1, B, G].
        ``dot=True`` adds the unrounded complex correlation at the maximum.  One ``npf_waveform_match_bank`` call (the rotation by
        the shift once per row, the contraction on the double-precision matrix instruction); inference only, no host sync, so a
        ``query`` and its ``match_bank`` can be captured in one graph (call once at the sizes before capturing: the workspace is
        allocated then)."""
        if self._y_dim != 2:
            raise ValueError(f"match_bank needs a model whose two outputs are (amplitude, phase): y_dim == 2, got {self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        if self._n_trgt is not None:
            raise ValueError("match_bank: the prediction carries n_trgt (padded targets), but a bank needs one shared grid: every "
                             "task must own all T points")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_match_bank_args((rows, T, ld), bank, weights, freqs, taus)
        if of == "samples":
            h = self._suff.detach().reshape(rows, T, ld)
        else:
            h = FN.mixture_summary(self._suff, n_z, self._y_dim, self._homosk)[0]
        want = ("match", "mismatch", "phase", "best_index", "best_match") + (("tau_index",) if taus is not None else ())
        m = FN.waveform_match_bank(h, bank, weights, freqs, taus, want=want, dot=dot)
        lead, G = (rows // B, B), bank.shape[0]
        tau = m.tau_index.double().mul_(float(taus[1])).add_(float(taus[0])).view(*lead, G) if taus is not None else None
        return BankMatch(m.match.view(*lead, G), m.mismatch.view(*lead, G), tau,
                         m.tau_index.view(*lead, G) if taus is not None else None, m.phase.view(*lead, G), m.best_index.view(lead),
                         m.best_match.view(lead), m.dot.view(*lead, G, 2) if dot else None)

    def loglike(self, data, weights=None, freqs=None, taus=None, of="samples", series=False) -> LogLike:
        """The matched-filter log likelihood ratio of the complex detector data ``data`` [B, T, 2] = (Re d, Im d) with the predicted
        waveform ``h = A e^{i phi}`` as the template -> :class:`LogLike`, for a model whose two outputs are (amplitude, phase).
        With ``<a|b> = sum_t w a conj(b)``, ``weights`` the caller's ``4 df / S_n(f)`` ([T] or [B, T]; ``None``: ones; a point whose
        weight is not in (0, inf) is removed) and ``taus = (tau0, dtau, n_tau)`` a grid of arrival times (``freqs`` in Hz carries the
        shift, with the sign of :meth:`match`): ``snr`` and ``lnl_max = max |<d|h>| - <h|h> / 2`` are maximised over the coalescence
        phase and the grid, ``lnl_marg = logsumexp_j (ln I0(|<d|h_j>|) - <h|h> / 2) - ln n_tau`` is marginalised over both with
        uniform priors, and ``lnl`` [B] is the log of the mean of ``exp(lnl_marg)`` over the latent samples: the model's own waveform
        uncertainty marginalised out of the likelihood (``lnl_max_mix``: the same of ``lnl_max``).  ``-<d|d> / 2`` is added to
        nothing; ``dd`` returns it.  Everything is float64: values reach 1e4 and differences of order 1 are what gets used.
        ``of="samples"``: on the raw decoder output, [n_z, B]; ``of="mean"``: the likelihood of the mixture-mean amplitude and
        phase (one moments-only ``npf_mixture_summary`` launch), [1, B], where ``lnl`` is that one row -- as it is for a
        deterministic model.  Padded targets (``n_trgt``) are left out.  ``series=True`` adds ``(L_j, SNR_j)`` over the grid.
        Two ``npf_waveform_loglike`` launches; inference only, no host sync, so a ``query`` and its ``loglike`` can be captured in
        one graph (call once at the sizes before capturing: the workspace is allocated then).
        Distance / amplitude marginalisation is :meth:`loglike_distance`, which returns this result as its ``base``.
        Inference only; the gradients of this likelihood, for training on ``ln Lambda``, come from its differentiable twin :meth:`lnl`.
        Out of scope: marginalising the head's per-point sigma (only the latent samples are marginalised);
        non-uniform time priors; sub-grid time interpolation."""
        if self._y_dim != 2:
            raise ValueError(f"loglike needs a model whose two outputs are (amplitude, phase): y_dim == 2, got {self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_loglike_args((rows, T, ld), data, weights, freqs, taus)
        with torch.no_grad():
            if of == "samples":
                h = self._suff.detach().reshape(rows, T, ld)
            else:
                h = FN.mixture_summary(self._suff, n_z, self._y_dim, self._homosk, n_valid=self._n_trgt)[0]
            want = tuple(k for k in FN.LOGLIKE_NAMES if k != "tau_index" or taus is not None)
            m = FN.waveform_loglike(h, data, weights, freqs, taus, n_valid=self._n_trgt, want=want, series=series)
            return _as_loglike(m, taus, (rows // B, B))

    def loglike_network(self, data, response, delays=None, weights=None, freqs=None, taus=None, of="samples",
                        series=False) -> NetworkLogLike:
        """The coherent matched-filter log likelihood ratio of the data of a network of ``D`` detectors, ``data`` [B, D, T, 2] =
        (Re d_k, Im d_k), with the predicted waveform as the template -> :class:`NetworkLogLike`.  Detector ``k`` sees ``C_k h``
        shifted by ``tau_j + delay_k`` under its own noise ``weights`` ([D, T] or [B, D, T]; ``None``: ones; a point whose weight is
        not in (0, inf) is removed for that detector): ``response`` [B, D, 2] = (Re C, Im C), the antenna pattern times the
        inclination factor, and ``delays`` [B, D] in seconds (either sign, not tied to the grid; ``None``: zeros) are float64 device
        tensors the host never reads.  The detectors' complex correlations ``<d_k|h>_k`` are added, each times ``C_k``, BEFORE the
        modulus is taken, and ``<h|h> = sum_k |C_k|^2 <h|h>_k``: one coalescence phase and one geocentric arrival time are shared by
        the network, which ``D`` calls of :meth:`loglike` cannot give (they maximise per detector and add moduli).  Everything else --
        ``freqs`` ([T] or [B, T], shared by the detectors, required with ``taus`` or ``delays``), ``taus``, ``of``, ``series``, the
        marginal over the latent samples, padded targets (``n_trgt``), float64 results -- is as in :meth:`loglike`; ``snr_det`` is
        each detector's own SNR at the network's grid time, ``optimal_snr_det = |C_k| sqrt(<h|h>_k)``.  Two
        ``npf_waveform_loglike_net`` launches; inference only, no host sync, so a ``query`` and its ``loglike_network`` can be
        captured in one graph (call once at the sizes before capturing) and replayed after ``response`` / ``delays`` were
        overwritten in place.  The distance marginalisation of this likelihood is :meth:`loglike_network_distance`.
        Inference only; the gradients of this likelihood come from its differentiable twin :meth:`lnl_network`.
        Out of scope: antenna patterns and delays from a sky position (the caller's, from their GW library); a sky grid per task;
        sub-grid time interpolation."""
        if self._y_dim != 2:
            raise ValueError(f"loglike_network needs a model whose two outputs are (amplitude, phase): y_dim == 2, got {self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_loglike_network_args((rows, T, ld), data, response, delays, weights, freqs, taus)
        with torch.no_grad():
            if of == "samples":
                h = self._suff.detach().reshape(rows, T, ld)
            else:
                h = FN.mixture_summary(self._suff, n_z, self._y_dim, self._homosk, n_valid=self._n_trgt)[0]
            want = tuple(k for k in FN.LOGLIKE_NET_NAMES if k != "tau_index" or taus is not None)
            m = FN.waveform_loglike_network(h, data, response, delays, weights, freqs, taus, n_valid=self._n_trgt, want=want,
                                            series=series)
            return _as_network_loglike(m, taus, (rows // B, B), response)

    def loglike_distance(self, data, scales, log_prior, weights=None, freqs=None, taus=None, of="samples",
                         posterior=False) -> DistanceLogLike:
        """:meth:`loglike` marginalised over the luminosity distance as well -> :class:`DistanceLogLike`.  The predicted waveform is
        the template at a reference distance ``d_ref``; at distance ``d`` it is ``a h`` with the amplitude scale ``a = d_ref / d``.
        ``scales`` (``a_i``) and ``log_prior`` (``ln pi_i``: the log prior MASS of grid point ``i``, quadrature weight included) are
        float64 device tensors [n_a] or [B, n_a] the host never reads (``functional.distance_prior`` makes both from a grid of
        distances).  A scale with ``a_i`` outside (0, inf) or a ``ln pi_i`` that is not finite is dead: it gets no mass and nothing
        else of it is used.  ``lnl_dist`` is the likelihood marginal over the coalescence phase, the grid of arrival times and the
        scale grid (the prior is not normalised: ``lnl_dist`` carries ``ln sum_i pi_i`` as given), ``lnl`` [B] its log-mean-exp over
        the latent samples; ``scale_hat = <d|h> / <h|h>`` at the maximum gives the maximum-likelihood distance ``d_ref /
        scale_hat`` and ``lnl_amp_max = snr ** 2 / 2`` the amplitude-maximised statistic; ``scale_index`` / ``scale_map`` are the
        grid point of the largest evidence.  ``posterior=True`` adds the log posterior mass of every scale: ``post`` per latent
        sample and ``post_mix`` [B, n_a] with the model's own waveform uncertainty marginalised out -- the distance posterior.
        Where no scale is live ``lnl_dist`` and every ``post`` are ``-inf`` and ``scale_index`` is 0; a task without live points or
        with a zero template has ``Lambda = 1`` at every scale, so its posterior is the normalised prior.  ``base`` is the
        :class:`LogLike` of :meth:`loglike` on the same inputs, bit for bit.  ``weights``, ``freqs``, ``taus``, ``of``, padded
        targets: as in :meth:`loglike`.  One correlation launch, the finishing launch of :meth:`loglike` and two
        ``npf_waveform_loglike_dist`` launches; inference only, no host sync, so a ``query`` and its ``loglike_distance`` can be
        captured in one graph (call once at the sizes before capturing) and replayed after ``scales`` / ``log_prior`` were
        overwritten in place.
        Out of scope: gradients; non-uniform time priors; marginalising the head's per-point sigma; continuous (non-grid) amplitude
        integration."""
        if self._y_dim != 2:
            raise ValueError(f"loglike_distance needs a model whose two outputs are (amplitude, phase): y_dim == 2, got {self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_loglike_distance_args((rows, T, ld), data, scales, log_prior, weights, freqs, taus)
        with torch.no_grad():
            h = self._waveform_rows(of, rows, ld)
            want = tuple(k for k in FN.LOGLIKE_NAMES if k != "tau_index" or taus is not None) + FN.LOGLIKE_DIST_NAMES
            m = FN.waveform_loglike_distance(h, data, scales, log_prior, weights, freqs, taus, n_valid=self._n_trgt, want=want,
                                             posterior=posterior)
            lead = (rows // B, B)
            return DistanceLogLike(*self._distance_fields(m, scales, lead), _as_loglike(m.base, taus, lead))

    def loglike_network_distance(self, data, response, delays, scales, log_prior, weights=None, freqs=None, taus=None, of="samples",
                                 posterior=False) -> NetworkDistanceLogLike:
        """:meth:`loglike_network` marginalised over the luminosity distance as well -> :class:`NetworkDistanceLogLike`: what
        :meth:`loglike_distance` computes, over the network sums -- one amplitude scale, one coalescence phase and one geocentric
        arrival time are shared by the detectors.  ``data``, ``response``, ``delays`` (``None``: zeros), ``weights``, ``freqs``,
        ``taus``, ``of``: as in :meth:`loglike_network`; ``scales``, ``log_prior``, ``posterior`` and the fields: as in
        :meth:`loglike_distance`; ``base`` is the :class:`NetworkLogLike` of :meth:`loglike_network` on the same inputs, bit for
        bit.  Inference only, no host sync; ``response``, ``delays``, ``scales`` and ``log_prior`` may be overwritten in place
        between the replays of a captured graph."""
        if self._y_dim != 2:
            raise ValueError("loglike_network_distance needs a model whose two outputs are (amplitude, phase): y_dim == 2, got "
                             f"{self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_loglike_distance_args((rows, T, ld), data, scales, log_prior, weights, freqs, taus, response, delays, network=True)
        with torch.no_grad():
            h = self._waveform_rows(of, rows, ld)
            want = tuple(k for k in FN.LOGLIKE_NET_NAMES if k != "tau_index" or taus is not None) + FN.LOGLIKE_DIST_NAMES
            m = FN.waveform_loglike_network_distance(h, data, response, delays, scales, log_prior, weights, freqs, taus,
                                                     n_valid=self._n_trgt, want=want, posterior=posterior)
            lead = (rows // B, B)
            return NetworkDistanceLogLike(*self._distance_fields(m, scales, lead), _as_network_loglike(m.base, taus, lead, response))

    def loglike_sky(self, data, response, delays, log_prior=None, weights=None, freqs=None, taus=None, of="samples", posterior=True,
                    snr_map=False) -> SkyLogLike:
        """:meth:`loglike_network` at every pixel of a sky grid, marginalised over the pixels -> :class:`SkyLogLike`: the sky map
        of an event under the predicted waveform in one call.  The grid is ONE grid shared by the tasks: ``response`` [P, D, 2] =
        (Re C, Im C) and ``delays`` [P, D] (seconds) hold every detector's response and arrival delay at every pixel, ``log_prior``
        [P] the log prior MASS of every pixel (``None``: uniform; not normalised here), all float64 device tensors the host never
        reads; a pixel whose ``log_prior`` is not finite is dead (no mass, ``-inf`` in ``post``, 0 in ``snr_map``).  ``lnl_sky``
        is the likelihood marginal over the coalescence phase, the grid of arrival times and the pixels, ``lnl`` [B] its
        log-mean-exp over the latent samples; ``pix_index`` is the pixel of the largest evidence and ``tau_index`` / ``tau`` /
        ``snr`` what :meth:`loglike_network` reports there.  ``posterior=True`` adds ``post`` (per latent sample) and
        ``post_mix`` [B, P], the sky posterior with the model's own waveform uncertainty marginalised out; ``snr_map=True`` the
        best SNR of every pixel.  ``freqs`` [T] is required, shared by all tasks (the pixel operand is), and must be finite.
        ``data``, ``weights``, ``taus``, ``of``, padded targets: as in :meth:`loglike_network`.  One
        ``npf_waveform_loglike_sky`` call: a complex GEMM with M = rows x n_tau, N = P, K = D T on the double-precision matrix
        instruction, three launches in place of ``2 P``; inference only, no host sync, so a ``query`` and its ``loglike_sky`` can
        be captured in one graph (call once at the sizes before capturing) and replayed after ``response`` / ``delays`` /
        ``log_prior`` were overwritten in place.
        Out of scope: antenna patterns and delays from (ra, dec, psi, iota), which come from the caller's GW library; a sky grid
        per task; gradients; adaptive or hierarchical pixel refinement (distance jointly with the sky: :meth:`loglike_sky_distance`)."""
        if self._y_dim != 2:
            raise ValueError(f"loglike_sky needs a model whose two outputs are (amplitude, phase): y_dim == 2, got {self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_loglike_sky_args((rows, T, ld), data, response, delays, log_prior, weights, freqs, taus)
        with torch.no_grad():
            h = self._waveform_rows(of, rows, ld)
            m = FN.waveform_loglike_sky(h, data, response, delays, log_prior, weights, freqs, taus, n_valid=self._n_trgt,
                                        posterior=posterior, snr_map=snr_map)
            lead, P = (rows // B, B), response.shape[0]
            tau = m.tau_index.double().mul_(float(taus[1])).add_(float(taus[0])).view(lead) if taus is not None else None
            return SkyLogLike(m.lnl_sky_mix, m.lnl_sky.view(lead), m.pix_index.view(lead),
                              m.tau_index.view(lead) if taus is not None else None, tau, m.snr.view(lead),
                              m.post.view(*lead, P) if posterior else None, m.post_mix,
                              m.snr_map.view(*lead, P) if snr_map else None)

    def loglike_sky_distance(self, data, response, delays, scales, log_prior_scale, log_prior=None, weights=None, freqs=None, taus=None,
                             of="samples", posterior=True, joint=False, moments=True) -> SkyDistanceLogLike:
        """:meth:`loglike_sky` marginalised over the amplitude scale of the template as well -> :class:`SkyDistanceLogLike`: the
        evidence marginal over phase, arrival time, sky position and distance, a sky map that assumes no distance (``post_sky``),
        a distance posterior that assumes no sky position (``post_dist``) and, per pixel, the conditional mean and spread of
        ``d / d_ref`` (``dist_mean``, ``dist_std``) that turn the sky map into a volume map.  ``response``, ``delays``,
        ``log_prior`` (the pixels' log prior mass), ``weights``, ``freqs``, ``taus``, ``of``, padded targets: as in
        :meth:`loglike_sky`; ``scales`` [n_a] and ``log_prior_scale`` [n_a]: as in :meth:`loglike_distance`
        (:func:`~npf_gwwaveform_amd.functional.distance_prior` makes both), but ONE grid shared by the tasks.  All are float64
        device tensors the host never reads.  ``posterior=True``: the two marginal posteriors and their mixtures over the
        latent samples; ``joint=True``: ``post_joint`` [.., B, P, n_a]; ``moments=True``: ``dist_mean`` / ``dist_std``.  One
        ``npf_waveform_loglike_sky_dist`` call, four launches in place of ``4 P``; inference only, no host sync, so a ``query``
        and its ``loglike_sky_distance`` can be captured in one graph (call once at the sizes before capturing) and replayed
        after the grids and priors were overwritten in place.
        Out of scope: gradients; per-task or per-pixel scale grids; moments of the mixture over the latent samples; antenna
        patterns from angles; adaptive pixel refinement; continuous amplitude integration."""
        if self._y_dim != 2:
            raise ValueError("loglike_sky_distance needs a model whose two outputs are (amplitude, phase): y_dim == 2, got "
                             f"{self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_loglike_sky_distance_args((rows, T, ld), data, response, delays, scales, log_prior_scale, log_prior, weights, freqs, taus)
        with torch.no_grad():
            h = self._waveform_rows(of, rows, ld)
            m = FN.waveform_loglike_sky_distance(h, data, response, delays, scales, log_prior_scale, log_prior, weights, freqs, taus,
                                                 n_valid=self._n_trgt, posterior=posterior, joint=joint, moments=moments)
            lead, P, n_a = (rows // B, B), response.shape[0], scales.shape[0]
            tau = m.tau_index.double().mul_(float(taus[1])).add_(float(taus[0])).view(lead) if taus is not None else None
            per = lambda t, *tail: t.view(*lead, *tail) if t is not None else None  # noqa: E731
            return SkyDistanceLogLike(m.lnl, m.lnl_vol.view(lead), m.pix_index.view(lead), m.scale_index.view(lead),
                                      scales.detach()[m.scale_index.view(lead).long()],
                                      m.tau_index.view(lead) if taus is not None else None, tau, m.snr.view(lead),
                                      m.scale_hat.view(lead), per(m.post_sky, P), per(m.post_dist, n_a), m.post_sky_mix,
                                      m.post_dist_mix, per(m.post_joint, P, n_a), per(m.dist_mean, P), per(m.dist_std, P))

    def _waveform_rows(self, of, rows, ld):
        """The (amplitude, phase) rows a likelihood is evaluated on: the raw decoder output or the mixture mean."""
        n_z, _, T = self.batch_shape
        if of == "samples":
            return self._suff.detach().reshape(rows, T, ld)
        return FN.mixture_summary(self._suff, n_z, self._y_dim, self._homosk, n_valid=self._n_trgt)[0]

    @staticmethod
    def _distance_fields(m, scales, lead):
        """The fields of :class:`DistanceLogLike` before ``base``, from a ``functional.WaveformLogLikeDistance``."""
        idx = m.scale_index.view(lead).long()
        grid = scales.detach()
        scale_map = grid[idx] if grid.dim() == 1 else grid.gather(1, idx.t()).t()  # ([B, n_a]: task b's own grid)
        n_a = scales.shape[-1]
        return (m.lnl_dist_mix, m.lnl_dist.view(lead), m.scale_hat.view(lead), m.lnl_amp_max.view(lead), m.scale_index.view(lead),
                scale_map, m.post.view(*lead, n_a) if m.post is not None else None, m.post_mix)

    def lnl(self, data, weights=None, freqs=None, taus=None, of="samples") -> Lnl:
        """The likelihoods of :meth:`loglike` (same arguments, same bits) as a training objective -> :class:`Lnl`: differentiable
        with respect to the raw decoder output, so ``(-p.lnl(d, ...).lnl).mean().backward()`` reaches the model's parameters --
        the surrogate is trained on the quantity it is used in.  Unlike the mismatch, ``ln Lambda`` sees amplitude errors; the
        gradient of ``lnl_marg`` and of the mixture ``lnl`` is exact, through the marginal over the grid of arrival times and over
        the latent samples; that of ``lnl_max`` / ``lnl_max_mix`` is taken at the grid time the forward found (a tie: the earlier
        one, a subgradient).  It flows into the amplitude and phase entries only: the scale entries of the raw output, padded
        targets (``n_trgt``), removed points and rows with ``<h|h> = 0`` receive exact zeros, so a loss made of the likelihood
        alone does not train sigma (:class:`~npf_gwwaveform_amd.losses.LogLikeLoss` adds a base loss for that).  ``of="mean"``:
        the likelihood of the mixture mean ([1, B]; one moments-only ``npf_mixture_summary`` launch); every latent sample receives
        ``1 / n_z`` of the task's gradient.  Forward: the launches of ``npf_waveform_loglike_ex``; backward: one
        ``npf_waveform_loglike_bwd`` launch.  No host sync: the call and its backward sit in a captured training step (call once
        at the sizes before capturing).  :meth:`loglike` stays the inference call: it returns everything else and builds no graph."""
        return self._lnl(None, data, None, None, weights, freqs, taus, of)

    def lnl_network(self, data, response, delays=None, weights=None, freqs=None, taus=None, of="samples") -> Lnl:
        """:meth:`lnl` of the coherent network likelihood: the values of :meth:`loglike_network` (same arguments, same bits),
        differentiable with respect to the raw decoder output (``npf_waveform_loglike_net_ex`` / ``npf_waveform_loglike_net_bwd``).
        No gradient reaches ``data``, ``response``, ``delays``, ``weights`` or ``freqs``."""
        return self._lnl("network", data, response, delays, weights, freqs, taus, of)

    def _lnl(self, network, data, response, delays, weights, freqs, taus, of) -> Lnl:
        who = "lnl_network" if network else "lnl"
        if self._y_dim != 2:
            raise ValueError(f"{who} needs a model whose two outputs are (amplitude, phase): y_dim == 2, got {self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        if network:
            FN.check_loglike_network_args((rows, T, ld), data, response, delays, weights, freqs, taus)
        else:
            FN.check_loglike_args((rows, T, ld), data, weights, freqs, taus)
        suff = self._suff.reshape(n_z * B, T, 4)
        extra = {}
        if of == "mean":
            extra = dict(n_bcast=n_z, mean=FN.mixture_summary(self._suff, n_z, self._y_dim, self._homosk, n_valid=self._n_trgt)[0])
        if network:
            m = FN.waveform_lnl_network(suff, data, response, delays, weights, freqs, taus, n_valid=self._n_trgt, **extra)
        else:
            m = FN.waveform_lnl(suff, data, weights, freqs, taus, n_valid=self._n_trgt, **extra)
        lead = (rows // B, B)
        return Lnl(m.lnl_mix, m.lnl_marg.view(lead), m.lnl_max.view(lead), m.lnl_max_mix)

    def mismatch(self, Y_ref, weights=None, freqs=None, taus=None, of="samples") -> torch.Tensor:
        """``mismatch`` of :meth:`match` (same arguments, same bits) as a training objective -> [n_z, B], or [1, B] for
        ``of="mean"``: differentiable with respect to the raw decoder output, so ``p.mismatch(Y).mean().backward()`` reaches the
        model's parameters.  The gradient is taken at the grid time the forward found (where two grid times tie: at the earlier one,
        a subgradient) and flows into the amplitude and phase entries only: the scale entries of the raw output, padded targets
        (``n_trgt``), removed points and degenerate rows receive exact zeros -- a loss made of the mismatch alone does not train
        sigma (:class:`~npf_gwwaveform_amd.losses.MismatchLoss` adds a likelihood for that).  ``of="mean"``: the mismatch of the
        mixture mean; the mean is linear in the samples' locs, so every latent sample receives ``1 / n_z`` of the task's gradient.
        Forward: the two ``npf_waveform_match_ex`` launches (after one moments-only ``npf_mixture_summary`` for the mean);
        backward: one ``npf_waveform_match_bwd`` launch.  No host sync: the call and its backward sit in a captured training step
        (call once at the sizes before capturing: the workspace is allocated then).  The raw decoder output is fp32 in the bf16
        compute mode as well (the head reads the same tensor), so the objective works there unchanged.  ``match`` stays the
        inference call: it returns everything else and builds no graph."""
        if self._y_dim != 2:
            raise ValueError(f"mismatch needs a model whose two outputs are (amplitude, phase): y_dim == 2, got {self._y_dim}")
        if of not in ("samples", "mean"):
            raise ValueError(f"of must be 'samples' or 'mean', got {of!r}")
        n_z, B, T = self.batch_shape
        rows, ld = (n_z * B, 4) if of == "samples" else (B, 2)
        FN.check_match_args((rows, T, ld), Y_ref, weights, freqs, taus)
        suff = self._suff.reshape(n_z * B, T, 4)
        if of == "samples":
            mm = FN.waveform_mismatch(suff, Y_ref, weights, freqs, taus, n_valid=self._n_trgt)
        else:
            mean = FN.mixture_summary(self._suff, n_z, self._y_dim, self._homosk, n_valid=self._n_trgt)[0]
            mm = FN.waveform_mismatch(suff, Y_ref, weights, freqs, taus, n_valid=self._n_trgt, n_bcast=n_z, mean=mean)
        return mm.view(rows // B, B)


class Conditioned:
    """A model conditioned on one context set (:meth:`NeuralProcessFamily.condition`): the encoded context points, their
    representation, and for a latent model q(z | C) with one draw of latent samples.  :meth:`query` evaluates the predictive
    distribution on any target grid from that state -- the context side is not run again and every query belongs to the same
    sampled functions ``z_samples``.  The model's parameters are read at query time: condition again after changing them."""

    def __init__(self, model, Xc_pt, R, z_samples, q_zCc, n_cntxt, B, C, fused_t, capacity=None, R_pts=None, eps=None):
        self._model, self._Xc_pt, self._R = model, Xc_pt, R
        self.z_samples, self.q_zCc = z_samples, q_zCc  # [n_z, B, 1, z_dim] and q(z | C); None for CNP / AttnCNP
        self.n_cntxt, self.B, self.C = n_cntxt, B, C
        self._fused_t = fused_t  # (decided at conditioning time: the context tensors were stored for that target side)
        # a growing context (``condition_with_capacity``): the state is stored at ``capacity`` rows per task, ``n_cntxt`` holds the live
        # device counts, ``_R_pts`` the per-point representations the pooled ``_R`` of CNP / LNP is refreshed from, ``eps`` the
        # standard-normal draw behind ``z_samples``; ``n_rows_bound``: what the host knows of the counts, an upper bound
        self.capacity, self._R_pts, self.eps = capacity, R_pts, eps
        self.n_rows_bound = C

    def query(self, X_trgt, n_trgt=None) -> HeadDistribution:
        """p(y | context, z) at ``X_trgt`` [B, T, x_dim] -> :class:`HeadDistribution` with batch shape [n_z, B, T]: the launches
        ``forward`` runs for its target side at these sizes (the masked route if the context was conditioned with ``n_cntxt``),
        with the stored latent samples.  ``n_trgt``: per-task target sizes of a padded grid, as in ``forward``.  Inference only
        (``torch.no_grad`` semantics), no host sync: a query and its ``summary`` can be captured in one graph."""
        m = self._model
        with torch.no_grad():
            if n_trgt is not None:
                n_trgt = m._check_counts(n_trgt, X_trgt, "n_trgt")
            m._check_tensors(X_trgt)
            if X_trgt.dim() != 3 or X_trgt.shape[0] != self.B:
                raise ValueError(f"X_trgt must be [B={self.B}, T, x_dim] (the batch the model was conditioned on), got {list(X_trgt.shape)}")
            if X_trgt.shape[1] == 0:
                raise ValueError("no target points")
            latent = (self.z_samples, self.q_zCc) if self.z_samples is not None else None
            n_keys = self.C if self.capacity is None else self.capacity  # (a growing context: always the padded route)
            return m._target_stage(self._Xc_pt, self._R, X_trgt, None, self.B, n_keys, self.n_cntxt, n_trgt, self._fused_t,
                                   latent=latent)[0]

    def extend(self, X_new, Y_new, n_new=None) -> "Conditioned":
        """Add observations to the context, in place -> ``self``.  ``X_new`` [B, N, x_dim], ``Y_new`` [B, N, y_dim]; ``n_new`` (integer
        device tensor [B], optional): task ``b`` adds its first ``n_new[b]`` rows only.  The per-point stages (x-encoder, XY-encoder)
        run on the ``N`` new points, one ``npf_append_points`` launch places them behind the rows every task holds and advances
        ``n_cntxt``, and what depends on the whole context is refreshed: the pooled representation of CNP / LNP, and for a latent
        model ``q_zCc`` and ``z_samples = loc + scale * eps`` with the stored ``eps`` (the same sampled functions, given more data).
        Every state tensor keeps its storage, so a captured ``extend`` followed by ``query`` replays.  Inference only, no host sync:
        the counts are never read by the host, which only keeps an upper bound of the rows offered (C + the sum of all ``N``, whatever
        ``n_new`` says) and raises ``ValueError`` when that exceeds ``capacity``."""
        m = self._model
        if self.capacity is None:
            raise ValueError("extend needs a growing context: condition with model.condition_with_capacity(..., capacity=M)")
        if X_new.dim() != 3 or X_new.shape[0] != self.B or X_new.shape[2] != m.x_dim:
            raise ValueError(f"X_new must be [B={self.B}, N, x_dim={m.x_dim}], got {list(X_new.shape)}")
        if Y_new.dim() != 3 or tuple(Y_new.shape[:2]) != tuple(X_new.shape[:2]) or Y_new.shape[2] != m.y_dim:
            raise ValueError(f"Y_new must be [B={self.B}, N={X_new.shape[1]}, y_dim={m.y_dim}], got {list(Y_new.shape)}")
        N = X_new.shape[1]
        if self.n_rows_bound + N > self.capacity:
            raise ValueError(f"extend: {self.n_rows_bound} rows offered so far + {N} new ones exceed capacity={self.capacity}")
        if N == 0:
            return self
        m._check_tensors(X_new, Y_new)
        if n_new is not None:
            n_new = FN.counts_i32(n_new, self.B, "n_new")
            if n_new.device != X_new.device:
                raise ValueError(f"n_new lives on {n_new.device}, the batch on {X_new.device}")
        with torch.no_grad():
            Xn_pt, Rn_pts = m._encode_points(X_new, Y_new)
            pairs = [(Rn_pts.t, self._R_pts.t, m.r_dim)]
            if self._Xc_pt is not None:
                pairs.append((Xn_pt.t, self._Xc_pt.t, m.x_transf_dim))
            FN.append_points(pairs, self.n_cntxt, n_new, self.B, N, self.capacity)
            self.n_rows_bound += N
            self._refresh()
        return self

    def _refresh(self):
        """What depends on the whole context, recomputed from the stored rows and the live counts, in place."""
        m = self._model
        if self._R is not self._R_pts:  # (CNP / LNP: the mean over the stored per-point representations)
            self._R.copy_(m._pool_pt(self._R_pts, self.B, n_valid=self.n_cntxt))
        if self.eps is not None:
            q = m._infer_q_zCc(self._R, self.B, self.n_cntxt).base_dist
            self.q_zCc.base_dist.loc.copy_(q.loc)
            self.q_zCc.base_dist.scale.copy_(q.scale)
            self.z_samples.copy_(q.loc + q.scale * self.eps)

    def rollout(self, X_trgt, eps=None, chunk=1) -> torch.Tensor:
        """One autoregressive sample of the function at ``X_trgt`` [B, T, x_dim] -> ``Y`` [B, T, y_dim]: for each block of ``chunk``
        targets in order, ``query`` the block, draw ``y = loc + scale * eps_block`` and ``extend`` the context by ``(x_block, y)`` --
        later targets are predicted given the earlier draws, which gives CNP / AttnCNP (whose one-shot predictive is a product of
        independent Gaussians) coherent samples.  ``eps`` [B, T, y_dim]: the standard-normal noise (default: one ``torch.randn`` draw).
        One trajectory per task: a latent model needs ``n_z == 1`` (tile the batch for several).  Needs ``capacity`` >= the rows
        offered so far + T.  NOTE: the state is left extended by the T drawn points -- a later ``query`` is conditioned on them."""
        m = self._model
        if self.capacity is None:
            raise ValueError("rollout needs a growing context: condition with model.condition_with_capacity(..., capacity=M)")
        if self.z_samples is not None and self.z_samples.shape[0] != 1:
            raise ValueError(f"rollout draws one trajectory per task: condition with n_z_samples=1 (got {self.z_samples.shape[0]})")
        if X_trgt.dim() != 3 or X_trgt.shape[0] != self.B or X_trgt.shape[2] != m.x_dim:
            raise ValueError(f"X_trgt must be [B={self.B}, T, x_dim={m.x_dim}], got {list(X_trgt.shape)}")
        T = X_trgt.shape[1]
        if eps is not None and tuple(eps.shape) != (self.B, T, m.y_dim):
            raise ValueError(f"eps must be [B={self.B}, T={T}, y_dim={m.y_dim}], got {list(eps.shape)}")
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be at least 1, got {chunk}")
        if self.n_rows_bound + T > self.capacity:
            raise ValueError(f"rollout: {self.n_rows_bound} rows offered so far + {T} targets exceed capacity={self.capacity}")
        m._check_tensors(X_trgt, eps)
        if eps is None:
            eps = torch.randn(self.B, T, m.y_dim, device=X_trgt.device)
        Y = torch.empty(self.B, T, m.y_dim, device=X_trgt.device)
        for s in range(0, T, chunk):
            x = X_trgt[:, s:s + chunk].contiguous()
            p = self.query(x).base_dist
            y = p.loc[0] + p.scale[0] * eps[:, s:s + chunk]
            Y[:, s:s + chunk] = y
            self.extend(x, y)
        return Y

    def loo(self) -> HeadDistribution:
        """The leave-one-out predictive of the stored context: for every context point ``i`` of every task, p(y_i | the task's other
        points) at ``x_i`` -> :class:`HeadDistribution` with batch shape [1, B, rows] (rows: ``capacity``, or C), whose target counts
        are the live context counts (rows beyond: ``loc = 0``, ``scale = 1``) -- see :meth:`NeuralProcessFamily.loo`.  Computed from
        the stored rows in one masked attention launch with the diagonal excluded (CNP: one ``npf_loo_mean`` launch) and the decoder;
        nothing is encoded again and the state is only read -- after ``extend`` the new points are included.  Accepted on states that
        hold the row tensors: every ``condition_with_capacity`` state, and ``condition`` states of attentive models that were not
        stored for the fused target side.  Inference only, no host sync."""
        m = self._model
        m._refuse_loo()
        if self.capacity is not None:
            Xc_pt, R_pts, rows, n = self._Xc_pt, self._R_pts, self.capacity, self.n_cntxt
        else:
            padded_kind = self.n_cntxt is not None and self.C > 0
            if not m._attentive:
                raise ValueError("loo: this context holds the pooled representation only; condition with a capacity "
                                 "(condition_with_capacity)")
            if self._fused_t and not padded_kind:
                raise ValueError("loo: this context was stored for the fused target side (images of keys / values only); "
                                 "condition with counts (n_cntxt=...) or a capacity (condition_with_capacity)")
            if self.C == 0:
                raise ValueError("loo: no context points")
            Xc_pt, R_pts, rows, n = self._Xc_pt, self._R, self.C, self.n_cntxt
        if Xc_pt is None or R_pts is None:
            raise ValueError("loo: this state does not hold the encoded context points and their representations")
        with torch.no_grad():
            if n is None:  # (conditioned without counts: every task holds all C rows)
                n = torch.full((self.B,), rows, dtype=torch.int32, device=Xc_pt.t.device)
            return m._loo_from(Xc_pt, R_pts, n, self.B, rows)

    def _rows(self) -> int:
        """Rows per task of the stored context: ``capacity``, or C."""
        return self.C if self.capacity is None else self.capacity

    def _row_tensors(self, what):
        """(encoded context points, per-point representations, live counts or None) of a state that holds the row tensors; the
        refusals of :meth:`sample_functions` for one that does not."""
        m = self._model
        if self.capacity is not None:
            Xc_pt, R_pts = self._Xc_pt, self._R_pts
        else:
            padded_kind = self.n_cntxt is not None and self.C > 0
            if self._fused_t and not padded_kind:
                raise ValueError(f"{what}: this context was stored for the fused target side (images of keys / values only); "
                                 "condition with counts (n_cntxt=...) or a capacity (condition_with_capacity)")
            if self.C == 0:
                raise ValueError(f"{what}: no context points")
            Xc_pt, R_pts = self._Xc_pt, (self._R if m._attentive else self._R_pts)
        if Xc_pt is None or R_pts is None:
            raise ValueError(f"{what}: this state does not hold the encoded context points and their representations")
        return Xc_pt, R_pts, self.n_cntxt

    def reweighted(self, W) -> "Reweighted":
        """S replicates of the stored context that differ in a non-negative weight per (replicate, task, context point) ->
        :class:`Reweighted`, whose :meth:`Reweighted.query` predicts from all of them at once.  ``W``: float device tensor
        [S, B, rows] (rows: ``capacity``, or C), used as given -- not copied if it is contiguous fp32, so weights overwritten in place
        are seen by a replayed graph.  In replicate ``s`` point ``i`` of task ``b`` counts ``W[s, b, i]`` times: softmax attention
        takes ``p_k ~ w_k exp(s_k)``, mean pooling ``sum w_k r_k / sum w_k`` (``npf_masked_attn_fwd_weighted`` /
        ``npf_weighted_mean``).  For integer weights the result is what ``forward`` gives on the context with its rows repeated; a
        weight of 0 (or a negative, NaN or Inf one) removes the point, and so does a row at or beyond the task's count.  The
        conditioned state is READ ONLY and stored once: nothing is encoded again, no key or value is copied per replicate.
        Accepted on the states :meth:`sample_functions` accepts: conditioned with a capacity, with ``n_cntxt``, or without counts if
        not stored for the fused target side.  Not implemented: ``is_self_attn=True`` and the bf16 compute mode.  No host sync."""
        m = self._model
        m._refuse_unimplemented("reweighted")
        rows = self._rows()
        if not isinstance(W, torch.Tensor) or not W.is_floating_point():
            raise ValueError(f"W must be a float device tensor [S, B={self.B}, rows={rows}], got "
                             f"{W.dtype if isinstance(W, torch.Tensor) else type(W).__name__}")
        if W.dim() != 3 or W.shape[0] < 1 or tuple(W.shape[1:]) != (self.B, rows):
            raise ValueError(f"W must be [S >= 1, B={self.B}, rows={rows}] (one weight per replicate, task and stored context row), "
                             f"got {list(W.shape)}")
        Xc_pt, R_pts, n = self._row_tensors("reweighted")
        if W.device != R_pts.t.device:
            raise ValueError(f"W lives on {W.device}, the conditioned state on {R_pts.t.device}")
        if W.requires_grad:
            raise RuntimeError("reweighted is inference only (no gradient flows to the weights): detach W")
        if n is None:  # (conditioned without counts: every task holds all C rows)
            n = torch.full((self.B,), rows, dtype=torch.int32, device=W.device)
        return Reweighted(self, W.to(torch.float32).contiguous(), Xc_pt, R_pts, n, rows)

    def bootstrap(self, X_trgt, n_samples, generator=None) -> HeadDistribution:
        """``reweighted(bootstrap_weights(n_cntxt, n_samples, rows, generator)).query(X_trgt)``: the predictions of ``n_samples``
        resamplings of every task's context points with replacement -> batch shape [n_z, n_samples * B, T], replicate-major.  Their
        spread is how much the prediction depends on which points happened to be observed."""
        S = int(n_samples)
        if S < 1:
            raise ValueError(f"n_samples must be at least 1, got {n_samples}")
        self._model._refuse_unimplemented("reweighted")
        rows = self._rows()
        _, R_pts, n = self._row_tensors("reweighted")
        dev = R_pts.t.device
        n = n if n is not None else torch.full((self.B,), rows, dtype=torch.int32, device=dev)
        return self.reweighted(bootstrap_weights(n, S, rows, generator=generator, device=dev)).query(X_trgt)

    def kfold(self, folds, k) -> HeadDistribution:
        """The k-fold predictive of the stored context: for every context point ``i`` of every task, p(y_i | the task's points of
        the OTHER folds) at ``x_i`` -> :class:`HeadDistribution` with batch shape [1, B, rows] whose target counts are the live
        context counts -- see :meth:`NeuralProcessFamily.kfold`.  From the stored rows: nothing is encoded again and the state is
        only read.  Accepted on the states :meth:`reweighted` accepts.  Inference only, no host sync."""
        m = self._model
        m._refuse_kfold()
        rows = self._rows()
        k = _check_folds(folds, k, self.B, rows)
        Xc_pt, R_pts, n = self._row_tensors("kfold")
        if folds.device != R_pts.t.device:
            raise ValueError(f"folds lives on {folds.device}, the conditioned state on {R_pts.t.device}")
        with torch.no_grad():
            if n is None:
                n = torch.full((self.B,), rows, dtype=torch.int32, device=folds.device)
            return m._kfold_from(Xc_pt, R_pts, n, folds, k, self.B, rows)

    def _function_sampler(self, X_trgt, n_samples, eps, chunk):
        """The argument checks of :meth:`sample_functions` -> (its per-call state, ``eps``, ``chunk``)."""
        m = self._model
        m._refuse_unimplemented("sample_functions")
        if self.z_samples is not None and self.z_samples.shape[0] != 1:
            raise ValueError(f"sample_functions draws one trajectory per sample: condition with n_z_samples=1 (got {self.z_samples.shape[0]})")
        if X_trgt.dim() != 3 or X_trgt.shape[0] != self.B or X_trgt.shape[2] != m.x_dim:
            raise ValueError(f"X_trgt must be [B={self.B}, T, x_dim={m.x_dim}], got {list(X_trgt.shape)}")
        T = X_trgt.shape[1]
        if T == 0:
            raise ValueError("X_trgt holds no target points")
        S = int(n_samples)
        if S < 1:
            raise ValueError(f"n_samples must be at least 1, got {n_samples}")
        if eps is not None and tuple(eps.shape) != (S, self.B, T, m.y_dim):
            raise ValueError(f"eps must be [S={S}, B={self.B}, T={T}, y_dim={m.y_dim}], got {list(eps.shape)}")
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be at least 1, got {chunk}")
        padded_kind = self.capacity is not None or (self.n_cntxt is not None and self.C > 0)
        if self._fused_t and not padded_kind:
            raise ValueError("sample_functions: this context was stored for the fused target side (images of keys / values only); "
                             "condition with counts (n_cntxt=...) or a capacity (condition_with_capacity)")
        m._check_tensors(X_trgt, eps)
        if eps is None:
            eps = torch.randn(S, self.B, T, m.y_dim, device=X_trgt.device)
        with torch.no_grad():
            return _FunctionSampler(self, S, T, X_trgt.device), eps, chunk

    def sample_functions(self, X_trgt, n_samples, eps=None, chunk=1) -> torch.Tensor:
        """``n_samples`` coherent function draws per task at ``X_trgt`` [B, T, x_dim] -> ``Y`` [S, B, T, y_dim]: sample ``s`` of task ``b``
        is what :meth:`rollout` returns for task ``b`` of a batch tiled S times, run with ``eps[s]`` (``eps`` [S, B, T, y_dim] standard
        normal, default one ``torch.randn`` draw; ``chunk`` as in ``rollout``).  The conditioned state is READ ONLY and stored once:
        the S x B trajectories (task ``s * B + b``) attend over / pool the shared context rows followed by a scratch tail of the points
        they drew themselves (T rows rounded up to whole tiles, owned by this call; ``npf_masked_attn_fwd_prefix``), so a later
        ``query`` / ``rollout`` / ``sample_functions`` sees the state as it was.  A latent model needs ``n_z == 1``; every sample
        recomputes q(z | C + its draws) with the state's ``eps``.  Accepts a state conditioned with a capacity, with ``n_cntxt``, or
        without counts if it was not stored for the fused target side.  Inference only, no host sync."""
        sampler, eps, chunk = self._function_sampler(X_trgt, n_samples, eps, chunk)
        S, B, T = sampler.S, self.B, X_trgt.shape[1]
        m = self._model
        Y = torch.empty(S, B, T, m.y_dim, device=X_trgt.device)
        with torch.no_grad():
            for t0 in range(0, T, chunk):
                x = X_trgt[:, t0:t0 + chunk]
                n = x.shape[1]
                x = x.unsqueeze(0).expand(S, B, n, m.x_dim).reshape(S * B, n, m.x_dim)
                y = sampler.step(x, eps[:, :, t0:t0 + chunk].reshape(S * B, n, m.y_dim))
                Y[:, :, t0:t0 + chunk] = y.view(S, B, n, m.y_dim)
        return Y


def tail_capacity(T: int) -> int:
    """Rows per task of the scratch tails of ``sample_functions``: the T drawn points rounded up to whole 32-point tiles."""
    return pad32(T)


def pooled_mean_of_two(mean_p, n_p, mean_t, n_t):
    """Mean over the union of two row sets from their means and sizes: ``(n_p mean_p + n_t mean_t) / max(n_p + n_t, 1)`` -- zeros where
    both are empty.  ``mean_*`` [..., r] float, ``n_*`` [...] integer (or float) counts, broadcast over the features."""
    n_p, n_t = n_p.to(mean_p.dtype).unsqueeze(-1), n_t.to(mean_t.dtype).unsqueeze(-1)
    return (n_p * mean_p + n_t * mean_t) / (n_p + n_t).clamp(min=1)


class _FunctionSampler:
    """The state of one ``Conditioned.sample_functions`` call: S x B tasks in sample-major order (task ``j = s * B + b`` reads prefix
    task ``j % B``) whose context is the conditioned state -- read only, stored once -- followed by a scratch tail of the points the
    task drew itself.  :meth:`step` is one autoregressive step (query a block, draw, append) without host sync or a change of any
    tensor's storage, so it can be captured in a graph and replayed block after block."""

    def __init__(self, post: "Conditioned", S: int, T: int, device):
        m = post._model
        self.post, self.m, self.S, self.B, self.SB = post, m, S, post.B, S * post.B
        B, r = post.B, m.r_dim
        self.c_pad = post.C if post.capacity is None else post.capacity
        self.m_tail = tail_capacity(T)
        if post.n_cntxt is not None:
            self.n_pre = post.n_cntxt  # (the live device counts: read by the kernels at every step)
        else:  # (conditioned without counts: every task holds all C rows)
            self.n_pre = torch.full((B,), self.c_pad, dtype=torch.int32, device=device)
        self.n_tail = torch.zeros(self.SB, dtype=torch.int32, device=device)
        zeros = lambda n, pts, F: torch.zeros(pt_shape(n, pts, F), device=device)  # noqa: E731
        att = getattr(m, "attender", None)
        latent = post.z_samples is not None
        # the tails ``npf_append_points`` fills, as (tensor, features): the per-point representations of the drawn points (the values
        # of scaled-dot attention, what CNP / LNP and the latent path of AttnLNP pool), then the attention's keys [and values]
        self.keep_R = not m._attentive or isinstance(att, DotAttender) or latent
        self.R_tail = zeros(self.SB, self.m_tail, r) if self.keep_R else None
        self.tails = [(self.R_tail, r)] if self.keep_R else []
        if m._attentive:
            Xc = post._Xc_pt.t if post._Xc_pt is not None else zeros(B, 0, m.x_transf_dim)
            R = post._R.t if post._R is not None else zeros(B, 0, r)
            if isinstance(att, DotAttender):
                self.K_tail = zeros(self.SB, self.m_tail, m.x_transf_dim)
                self.tails.append((self.K_tail, m.x_transf_dim))
                self.walk = PrefixTail(Xc, R, self.n_pre, self.K_tail, self.R_tail, self.n_tail, B, self.c_pad, self.m_tail)
            else:  # learned projections: the prefix projected and split into heads once, the tails hold projected rows
                H, d = att.n_heads, att.kq_size
                if self.c_pad > 0:
                    Kh = FN.split_heads(att._project(Xc, B, self.c_pad, att.key_transform), B, self.c_pad, d, H)
                    Vh = FN.split_heads(att._project(R, B, self.c_pad, att.value_transform), B, self.c_pad, att.value_size, H)
                else:  # (conditioned on no context at all: an empty prefix, nothing to project)
                    Kh, Vh = zeros(H * B, 0, d // H), zeros(H * B, 0, att.value_size // H)
                self.K_tail, self.V_tail = zeros(self.SB, self.m_tail, d), zeros(self.SB, self.m_tail, att.value_size)
                self.tails += [(self.K_tail, d), (self.V_tail, att.value_size)]
                self.walk = PrefixTail(Kh, Vh, self.n_pre, self.K_tail, self.V_tail, self.n_tail, H * B, self.c_pad, self.m_tail,
                                       heads_of_prefix=H)
            # the pooled prefix representation of the latent path (AttnLNP)
            self.mean_pre = FN.masked_mean(R, self.n_pre, B, self.c_pad, r)[:, :r] if (latent and self.c_pad > 0) \
                else torch.zeros(B, r, device=device)
        else:
            self.walk = None
            self.mean_pre = post._R.reshape(B, r)  # (CNP / LNP keep the pooled mean of the context)
        self.eps_z = None
        if latent:
            if post.eps is not None:
                eps = post.eps
            else:  # (``condition`` keeps z, not the draw behind it: the same draw, from z = loc + scale * eps)
                q = post.q_zCc.base_dist
                eps = (post.z_samples - q.loc) / q.scale
            self.eps_z = eps[0].repeat(S, 1, 1)  # [S B, 1, z]: every sample of task b is drawn with the state's eps of task b

    def _pooled(self):
        """[S B, 1, r]: the mean representation over each task's prefix and tail rows."""
        m, r = self.m, self.m.r_dim
        mean_t = FN.masked_mean(self.R_tail, self.n_tail, self.SB, self.m_tail, r)[:, :r]
        n_p = self.n_pre.clamp(0, self.c_pad).repeat(self.S)
        return pooled_mean_of_two(self.mean_pre.repeat(self.S, 1), n_p, mean_t, self.n_tail).reshape(self.SB, 1, r)

    def step(self, x, eps):
        """``x`` [S B, n, x_dim], ``eps`` [S B, n, y_dim] -> ``y`` [S B, n, y_dim] drawn given each task's context and earlier draws;
        the tails grow by the n points."""
        m, SB = self.m, self.SB
        n = x.shape[1]
        Xt_pt = m._xenc_pt(x)
        z = None
        R = None
        if self.eps_z is not None or not m._attentive:
            R = self._pooled()
        if self.eps_z is not None:
            q = m._latent_dist_from(R).base_dist
            z = (q.loc + q.scale * self.eps_z).unsqueeze(0)  # [1, S B, 1, z]
        C = self.c_pad + self.m_tail
        if m._attentive:
            suff = m._target_suffstat(None, z, None, Xt_pt, SB, C, n, n_valid=self.walk)
        else:
            suff = m._target_suffstat(None, z, R, Xt_pt, SB, C, n)
        p = m._head(suff, None, SB, n).base_dist
        y = p.loc[0] + p.scale[0] * eps
        Xn_pt, Rn_pts = m._encode_points(x, y)
        src = [Rn_pts.t] if self.keep_R else []
        if m._attentive:
            att = m.attender
            if isinstance(att, DotAttender):
                src.append(Xn_pt.t)
            else:
                src += [att._project(Xn_pt.t, SB, n, att.key_transform), att._project(Rn_pts.t, SB, n, att.value_transform)]
        FN.append_points([(s, dst, F) for s, (dst, F) in zip(src, self.tails)], self.n_tail, None, SB, n, self.m_tail)
        return y


class Reweighted:
    """S replicates of one conditioned context that differ in a weight per (replicate, task, context point)
    (:meth:`Conditioned.reweighted`).  Holds the weights ``W`` [S, B, rows] (the caller's tensor if it was contiguous fp32: overwrite
    it in place and query again, or replay a captured query) and reads the conditioned state, which stays as it is."""

    def __init__(self, post: "Conditioned", W, Xc_pt, R_pts, n, rows):
        self.post, self.W, self.S, self.B, self.rows = post, W, W.shape[0], post.B, rows
        self._Xc_pt, self._R_pts, self.n_cntxt = Xc_pt, R_pts, n

    def _eps(self):
        """[n_z, S B, 1, z]: every replicate of task b is drawn with the state's eps of task b (the rule of ``sample_functions``)."""
        post = self.post
        if post.eps is not None:
            eps = post.eps
        else:  # (``condition`` keeps z, not the draw behind it: the same draw, from z = loc + scale * eps)
            q = post.q_zCc.base_dist
            eps = (post.z_samples - q.loc) / q.scale
        return eps.repeat(1, self.S, 1, 1)

    def query(self, X_trgt, n_trgt=None) -> HeadDistribution:
        """p(y | replicate s of the context, z) at ``X_trgt`` [B, T, x_dim] (shared by the replicates) -> :class:`HeadDistribution`
        with batch shape [n_z, S * B, T], replicate-major (task ``s * B + b``, the order of ``sample_functions``); ``n_trgt`` [B]:
        per-task target sizes of a padded grid, repeated per replicate.  CNP: ``npf_weighted_mean``, then the decoder per (replicate,
        task); AttnCNP: ``npf_masked_attn_fwd_weighted`` over the one stored copy of keys / values, then the decoder of the padded
        route; LNP / AttnLNP: q(z | replicate) from the weighted mean of the per-point representations and ``z = loc + scale * eps``
        with the state's ``eps`` of task ``b`` for every replicate (the state's ``n_z`` draws are kept), then merge and decode over
        the S * B tasks.  A replicate without an admissible point is predicted from the empty context.  ``summary`` and ``score``
        work on the result as on any other.  Inference only, no host sync: a query and its ``summary`` can be captured in one graph
        and replayed after ``W`` was overwritten in place."""
        post, m, S, B, rows = self.post, self.post._model, self.S, self.B, self.rows
        SB, r = S * B, m.r_dim
        with torch.no_grad():
            if n_trgt is not None:
                n_trgt = m._check_counts(n_trgt, X_trgt, "n_trgt").repeat(S)
            m._check_tensors(X_trgt)
            if X_trgt.dim() != 3 or X_trgt.shape[0] != B:
                raise ValueError(f"X_trgt must be [B={B}, T, x_dim] (the batch the model was conditioned on), got {list(X_trgt.shape)}")
            T = X_trgt.shape[1]
            if T == 0:
                raise ValueError("no target points")
            Xt_pt = m._xenc_pt(X_trgt)
            z = Rw = None
            if post.z_samples is not None or not m._attentive:
                Rw = FN.weighted_mean(self._R_pts.t, self.W, self.n_cntxt, SB, B, rows, r)[:, :r].reshape(SB, 1, r)
            if post.z_samples is not None:
                q = m._latent_dist_from(Rw).base_dist
                z = q.loc.unsqueeze(0) + q.scale.unsqueeze(0) * self._eps()  # [n_z, S B, 1, z]
            if m._attentive:
                # (the decoder, and the residual of a transformer attender, read the encoded targets per task: tiled; the attention
                # itself reads those of the first replicate)
                Xt_rep = PTensor(Xt_pt.t.repeat(S, 1, 1, 1, 1), T, m.x_transf_dim) if S > 1 else Xt_pt
                suff = m._target_suffstat(self._Xc_pt, z, self._R_pts, Xt_rep, SB, rows, T,
                                          n_valid=KeyWeights(self.W, self.n_cntxt, S), n_q_valid=n_trgt)
            else:
                vec = Rw.reshape(SB, r) if z is None else m._rep_rows(z, Rw, SB)
                suff = m._decode_taskvec(Xt_pt, vec.contiguous(), B, T, vec.shape[0])
            return m._head(suff, None, SB, T, n_trgt=n_trgt)


def bootstrap_weights(n_cntxt_or_C, S, rows, generator=None, device=None, n_tasks=1) -> torch.Tensor:
    """Bootstrap multiplicities [S, B, rows] (fp32) for :meth:`Conditioned.reweighted`: for every (s, b), ``n[b]`` draws with
    replacement among the first ``n[b]`` rows -- row ``i`` holds how often it was drawn -- and 0 beyond.  ``n_cntxt_or_C``: the
    per-task counts, an integer tensor [B] (clamped to [0, rows]; never read by the host), or one host int C for each of ``n_tasks``
    tasks.  ``generator``: a ``torch.Generator`` of ``device`` (default: the counts' device).  No host sync."""
    S, rows = int(S), int(rows)
    if S < 1 or rows < 1:
        raise ValueError(f"bootstrap_weights needs S >= 1 and rows >= 1, got {S} and {rows}")
    if isinstance(n_cntxt_or_C, torch.Tensor):
        n = n_cntxt_or_C
        if n.dim() != 1 or n.is_floating_point() or n.dtype == torch.bool:
            raise ValueError(f"the counts must be an integer tensor [B], got {n.dtype} {list(n.shape)}")
        device = n.device if device is None else torch.device(device)
        n = n.to(device)
    else:
        n = torch.full((int(n_tasks),), int(n_cntxt_or_C), dtype=torch.int32, device=device)
        device = n.device
    B = n.shape[0]
    n = n.clamp(0, rows).view(1, B, 1)
    u = torch.rand(S, B, rows, generator=generator, device=device)
    idx = (u * n).long().minimum((n - 1).clamp(min=0).long())  # draw j of (s, b): uniform on the first n[b] rows
    drawn = (torch.arange(rows, device=device).view(1, 1, rows) < n).to(torch.float32).expand(S, B, rows)  # (the first n[b] draws count)
    return torch.zeros(S, B, rows, dtype=torch.float32, device=device).scatter_add_(2, idx, drawn.contiguous())


def _check_folds(folds, k, B, rows) -> int:
    k = int(k)
    if k < 2:
        raise ValueError(f"k must be at least 2 folds, got {k}")
    if not isinstance(folds, torch.Tensor) or folds.is_floating_point() or folds.dtype == torch.bool:
        raise ValueError(f"folds must be an integer tensor [B={B}, rows={rows}] of fold ids in [0, k), got "
                         f"{folds.dtype if isinstance(folds, torch.Tensor) else type(folds).__name__}")
    if tuple(folds.shape) != (B, rows):
        raise ValueError(f"folds must be [B={B}, rows={rows}] (one fold id per stored context row), got {list(folds.shape)}")
    return k


def kfold_weights(folds, k) -> torch.Tensor:
    """``W[f, b, i] = (folds[b, i] != f)`` as fp32 [k, B, rows]: replicate ``f`` is the context without the points of fold ``f``."""
    return (folds.unsqueeze(0) != torch.arange(int(k), device=folds.device, dtype=folds.dtype).view(-1, 1, 1)).to(torch.float32)


def _mean_rows(R_pt, pts, B, r, n_valid=None):
    """Row-major [B, 1, r]: the mean over the ``pts`` points of every task of a PT32 tensor, or over the first ``n_valid[b]`` of them,
    or (``n_valid`` a :class:`TrainKeyWeights`) their weighted mean."""
    if isinstance(n_valid, TrainKeyWeights):  # (a weight per point, with gradients: forward(w_cntxt=...))
        m = FN.key_weighted_mean(R_pt, n_valid.w, n_valid.n_valid, B, pts, r)
    else:
        m = FN.mean_agg(R_pt, pts, r) if n_valid is None else FN.masked_mean(R_pt, n_valid, B, pts, r)
    return m[:, :r].reshape(B, 1, r)


def _q_z_scale(z_scale):
    return 0.1 + 0.9 * torch.sigmoid(z_scale)


class NeuralProcessFamily(nn.Module, abc.ABC):
    """Base class (npf/neuralproc/base.py:23-371)."""

    _valid_paths = ["deterministic", "latent", "both"]

    def __init__(self, x_dim, y_dim, encoded_path, r_dim=128, x_transf_dim=-1, is_heteroskedastic=True, XEncoder=None,
                 Decoder=None, PredictiveDistribution=MultivariateNormalDiag, p_y_loc_transformer=None,
                 p_y_scale_transformer=None):
        super().__init__()
        self.x_dim, self.y_dim, self.r_dim = x_dim, y_dim, r_dim
        self.is_heteroskedastic = is_heteroskedastic
        if x_transf_dim is None:
            self.x_transf_dim = self.x_dim
        elif x_transf_dim == -1:
            self.x_transf_dim = self.r_dim
        else:
            self.x_transf_dim = x_transf_dim
        self.encoded_path = encoded_path.lower()
        if self.encoded_path not in self._valid_paths:
            raise ValueError(f"Unknown encoded_path={self.encoded_path}.")
        if PredictiveDistribution is not MultivariateNormalDiag or p_y_loc_transformer is not None \
                or p_y_scale_transformer is not None:
            raise NotImplementedError("the HIP Gaussian head implements the reference defaults only: diagonal "
                                      "Gaussian, identity loc, scale = 0.01 + 0.99 softplus (base.py:114-116)")
        if XEncoder is None:
            XEncoder = self.dflt_Modules["XEncoder"]
        if Decoder is None:
            Decoder = self.dflt_Modules["Decoder"]
        self.x_encoder = XEncoder(self.x_dim, self.x_transf_dim)
        self.decoder = Decoder(self.x_transf_dim, self.r_dim, self.y_dim * 2)
        if not isinstance(self.x_encoder, MLP) or not isinstance(self.decoder, MergeFlatInputs):
            raise NotImplementedError("the HIP path needs the stock MLP XEncoder and merge_flat_input(MLP) Decoder")
        if max(self.x_dim, 2 * self.y_dim) > 32:
            raise NotImplementedError("x_dim and 2*y_dim are limited to 32 on the hot path")
        self.PredictiveDistribution = PredictiveDistribution
        self.p_y_loc_transformer = nn.Identity()
        self.validate_inputs = True

    def reset_parameters(self):  # no-op in the reference as well
        pass

    @property
    def dflt_Modules(self):
        d = dict()
        d["XEncoder"] = partial(MLP, n_hidden_layers=1, hidden_size=self.r_dim)
        d["SubDecoder"] = partial(MLP, n_hidden_layers=4, hidden_size=self.r_dim)
        d["Decoder"] = merge_flat_input(d["SubDecoder"], is_sum_merge=True)
        return d

    # ------------------------------------------------------------------ forward
    def forward(self, X_cntxt, Y_cntxt, X_trgt, Y_trgt=None, n_cntxt=None, n_trgt=None):
        """Same contract as base.py:177-239: returns ``(p_yCc, z_samples, q_zCc, q_zCct)``.

        ``n_cntxt``: per-task context sizes of a PADDED batch -- an integer device tensor [B] (int32 or int64), task ``b`` uses
        the rows ``X_cntxt[b, :n_cntxt[b]]`` / ``Y_cntxt[b, :n_cntxt[b]]`` and everything returned for it equals what the
        single-task batch cut to those rows returns.  The counts are read by the kernels only (no host sync): a step captured
        in a graph is replayed with new counts.  The rows beyond the count have no influence on any output or gradient, but the
        training-time range check covers them too: padding must be finite and inside [-1, 1] (fill it with zeros).  ``X_cntxt``
        with zero rows behaves as without ``n_cntxt``.  Not implemented with ``n_cntxt``: self-attention context encoders
        (``is_self_attn=True``) and the bf16 compute mode.

        ``n_trgt``: the same for the targets -- an integer device tensor [B], task ``b`` owns the rows ``X_trgt[b, :n_trgt[b]]`` /
        ``Y_trgt[b, :n_trgt[b]]``.  For every row ``t < n_trgt[b]`` everything returned equals what the single-task batch cut to
        those target rows (and, with ``n_cntxt``, those context rows) returns; the per-task loss (the returned distribution carries
        the counts: ``criterion(out, Y_trgt)`` as always) and every parameter gradient equal those of the cut batch.  Rows
        ``t >= n_trgt[b]`` have no influence on any row below the count, on the loss or on any gradient; their ``loc`` is 0 and
        their ``scale`` 1.  The padding must be finite and, in training, inside [-1, 1] (fill it with zeros).  ``n_trgt[b] == 0``
        is allowed: that task's log-likelihood is 0 and it contributes no gradient.  Read by the kernels only, like ``n_cntxt``:
        one captured step serves every mix of both counts.  Without ``n_cntxt`` the step keeps its path (padded targets are just
        points to the per-point stages); what ties a task's targets together -- the head and the loss, the homoskedastic pooling,
        the target-side mean of the latent path -- reads the counts.  With ``n_cntxt`` the masked attention also skips the
        queries beyond the count.  Not implemented with ``n_trgt``: ``is_self_attn=True`` and the bf16 compute mode.

        The conditional models (CNP, AttnCNP) also take ``w_cntxt``, a weight per context point: :meth:`_forward_weighted`."""
        return self._forward_weighted(X_cntxt, Y_cntxt, X_trgt, Y_trgt, n_cntxt=n_cntxt, n_trgt=n_trgt)

    def _forward_weighted(self, X_cntxt, Y_cntxt, X_trgt, Y_trgt=None, n_cntxt=None, n_trgt=None, w_cntxt=None):
        """``forward`` with one more argument; it IS the ``forward`` of CNP and AttnCNP (the base class keeps the reference's
        argument list plus the counts).

        ``w_cntxt``: a weight per context point -- a float device tensor [B, C] that may require grad.  Point ``k`` of task ``b``
        enters what ties the points of a task together with weight ``w_cntxt[b, k]``: the mean of CNP becomes
        ``sum_k w_k r_k / sum_k w_k`` (``functional.key_weighted_mean``), the attention of AttnCNP ``p_k ~ w_k exp(s_k)``
        (``functional.key_weighted_attention``; scaled-dot, multihead and transformer attention, the weights shared by the heads).
        With C > 0 the step takes the padded route; ``n_cntxt=None`` then means that every row lies below the count, and ``n_trgt``
        combines with it as with ``n_cntxt``.  A point is removed unless ``0 < w < inf`` (a weight that is 0, negative, NaN or Inf
        removes it, whatever its row holds after the per-point encoders), integer weights give what ``forward`` gives on the context
        with its rows repeated, and all-ones weights give the bits of the ``n_cntxt`` forward.  Everything is differentiable in the
        weights too: ``w_cntxt.grad`` of a removed point, or beyond the count, is an exact zero (no one-sided derivative at
        ``w = 0``); see :meth:`influence`.  The range check does not look at the weights, and nothing reads them on the host: a
        captured step sees weights overwritten in place.  Not implemented with ``w_cntxt``: ``is_self_attn=True``, the bf16
        compute mode and the latent models (LNP / AttnLNP: q(z | C, T) would need a rule for the targets' weights)."""
        if n_cntxt is not None:
            n_cntxt = self._check_counts(n_cntxt, X_cntxt, "n_cntxt")
        if n_trgt is not None:
            n_trgt = self._check_counts(n_trgt, X_trgt, "n_trgt")
        if w_cntxt is not None:
            w_cntxt = self._check_weights(w_cntxt, X_cntxt)
        self._validate_inputs(X_cntxt, Y_cntxt, X_trgt, Y_trgt)
        B, C, _ = X_cntxt.shape
        T = X_trgt.shape[1]
        if T == 0:
            raise ValueError("no target points")
        if w_cntxt is not None and C > 0:
            # (the counts' place on the padded route: the kernels that tie a task's points together read the weights with them)
            full = n_cntxt if n_cntxt is not None else torch.full((B,), C, dtype=torch.int32, device=X_cntxt.device)
            n_cntxt = TrainKeyWeights(w_cntxt, full)
        fused_t = self._fused_target_side(C, T)
        Xc_pt, R = self._context_stage(X_cntxt, Y_cntxt, n_cntxt, fused_t)
        return self._target_stage(Xc_pt, R, X_trgt, Y_trgt, B, C, n_cntxt, n_trgt, fused_t)

    def influence(self, X_cntxt, Y_cntxt, X_trgt, Y_trgt, n_cntxt=None, n_trgt=None) -> torch.Tensor:
        """[B, C]: the gradient of every task's summed target log-likelihood ``log p(Y_trgt[b] | context b)`` with respect to the
        weight of each of its context points at ``w_cntxt = 1`` -- the infinitesimal jackknife: how much each observed point drives
        the prediction, for every point from one forward and one backward pass (``bootstrap`` / ``kfold`` estimate it by
        predicting again per replicate).  ``n_cntxt`` / ``n_trgt`` as in ``forward``; zeros at and beyond ``n_cntxt[b]``.  Runs in
        eval mode (restored afterwards) and through ``torch.autograd.grad`` on the weights alone: no parameter's ``.grad`` is
        touched.  Refused where ``forward(w_cntxt=...)`` is."""
        self._refuse_weights()
        B, C, _ = X_cntxt.shape
        w = torch.ones((B, C), dtype=torch.float32, device=X_cntxt.device, requires_grad=True)
        if C == 0:
            return w.detach()
        was = self.training
        self.eval()
        try:
            with torch.enable_grad():
                p_yCc = self(X_cntxt, Y_cntxt, X_trgt, Y_trgt, n_cntxt=n_cntxt, n_trgt=n_trgt, w_cntxt=w)[0]
                ll = p_yCc.sum_log_prob(Y_trgt)  # [n_z = 1, B]
                (g,) = torch.autograd.grad(ll.sum(), w)
        finally:
            self.train(was)
        return g

    def _context_stage(self, X_cntxt, Y_cntxt, n_cntxt, fused_t):
        """Everything ``forward`` runs before it touches the targets -> (encoded context points ``Xc_pt``, representation ``R``).
        ``n_cntxt`` (device int32 [B], with C > 0): the padded route -- the per-point stages -- x-encoder, XY-encoder, over all rows
        of the padded context -- keep the launches of an unfused step; what ties the points of a task together (the mean over the
        context here, the attention in ``_target_stage``) runs on the masked kernels (csrc/masked_kernels.hip).  ``fused_t``: will
        the target side be one x6 program (``_fused_target_side``; it decides which companion copies of keys / values the chain
        launches store)."""
        from . import chain as _chain

        B, C, _ = X_cntxt.shape
        if n_cntxt is not None and C > 0:
            if self._fused_context_side(C):
                from . import x6

                Xc_pt, R_pts = x6.context_side(self, X_cntxt, Y_cntxt)
                return Xc_pt, self._pool_pt(R_pts, B, n_valid=n_cntxt)
            Xc_pt = self._xenc_pt(X_cntxt)
            return Xc_pt, self._encode_globally_pt(Xc_pt, Y_cntxt, B, C, n_valid=n_cntxt)
        fused_c = self._fused_context_side(C)
        if fused_c and self._attentive and not fused_t and _chain.COMPUTE_DTYPE == "bf16":
            fused_c = False  # (the bf16 attention chain streams the bf16 images of keys / values its producer chains store)
        if fused_c:
            # x-encoder + XY-encoder of the context points as one x6 program (x6.py); the pooling stays the subclass's
            from . import x6

            Xc_pt, R_pts = x6.context_side(self, X_cntxt, Y_cntxt)
            return Xc_pt, self._pool_pt(R_pts, B)
        Xc_pt = self._xenc_pt(X_cntxt, with_tr=self._attentive and not fused_t) if C > 0 else None
        return Xc_pt, self._encode_globally_pt(Xc_pt, Y_cntxt, B, C)

    def _target_stage(self, Xc_pt, R, X_trgt, Y_trgt, B, C, n_cntxt, n_trgt, fused_t, latent=None):
        """The rest of ``forward`` from what ``_context_stage`` returned -> ``(p_yCc, z_samples, q_zCc, q_zCct)``.  ``latent``:
        ``(z_samples, q_zCc)`` drawn earlier (a conditioned model, :meth:`condition`) instead of the latent path here.  On the padded
        route (``n_cntxt`` with C > 0) the fused target side (x6.target_side) is not taken: its softmax has the key count as a launch
        argument.  With ``n_trgt`` the masked attention then skips the queries beyond the count, and on either route the head / the
        target-side mean of the latent path read it."""
        T = X_trgt.shape[1]
        padded = n_cntxt is not None and C > 0
        n_valid = n_cntxt if padded else None
        X_raw = None
        if padded:
            Xt_pt = self._xenc_pt(X_trgt)
        elif fused_t:
            Xt_pt, X_raw = None, X_trgt  # (the target side runs as one x6 program from the raw features)
        elif self._xenc_with_query_projection(C, T):
            # multihead / transformer attention with 16-wide heads: the target x-encoder and the attender's query projection as
            # one x6 program (x6.xenc_proj)
            from . import x6

            Xt_pt, q_proj = x6.xenc_proj(self, X_trgt, self.attender.query_transform)
            Xt_pt.proj = q_proj
        else:
            Xt_pt = self._xenc_pt(X_trgt)
        self._X_trgt_raw = X_raw  # (per-call: read by the two methods below only)
        try:
            if latent is not None:
                z_samples, q_zCc, q_zCct = latent[0], latent[1], None
            elif self.encoded_path in ["latent", "both"]:
                z_samples, q_zCc, q_zCct = self._latent_path_pt(R, C, Xt_pt, Y_trgt, B, T, n_valid=n_valid, n_trgt=n_trgt)
            else:
                z_samples, q_zCc, q_zCct = None, None, None
            if self.encoded_path == "latent":
                R = None
            suff = self._target_suffstat(Xc_pt, z_samples, R, Xt_pt, B, C, T, n_valid=n_valid,
                                         n_q_valid=n_trgt if padded else None)  # [n_z * B, T, 2 dy]
        finally:
            self._X_trgt_raw = None
        return self._head(suff, Y_trgt, B, T, n_trgt=n_trgt), z_samples, q_zCc, q_zCct

    # ------------------------------------------------------------------ conditioned prediction
    def _n_z_for(self, n_z_samples=None) -> Optional[int]:
        """Latent samples of an inference call (None: not a latent model)."""
        return None

    def condition(self, X_cntxt, Y_cntxt, n_cntxt=None, n_z_samples=None) -> "Conditioned":
        """Encode the context once: everything ``forward`` runs before it first touches the targets, on the kernels ``forward`` would
        take for this context size (``n_cntxt``: the padded route, as in ``forward``), and for a latent model q(z | C) and ONE draw
        of ``n_z_samples`` latent samples (default: ``n_z_samples_test`` / ``n_z_samples_train`` by the model's mode).  The returned
        :class:`Conditioned` answers any number of :meth:`Conditioned.query` calls from that state: every grid queried belongs to
        the same sampled functions.  Inference only (``torch.no_grad`` semantics, the model's train / eval mode respected); no host
        sync, so the training-time [-1, 1] range check is not applied."""
        with torch.no_grad():
            n_z = self._n_z_for(n_z_samples)
            if n_cntxt is not None:
                n_cntxt = self._check_counts(n_cntxt, X_cntxt, "n_cntxt")
            self._check_tensors(X_cntxt, Y_cntxt)
            B, C, _ = X_cntxt.shape
            if n_z is not None:
                self.n_z_samples = n_z  # (read by AttnLNP's dispatch rule; ``query`` uses what is stored below, not this attribute)
            fused_t = self._fused_target_side(C, 1)  # (the rule does not depend on the number of targets: x6.target_side_usable)
            R_pts = None
            if not self._attentive and C > 0 and not getattr(self, "is_self_attn", False):
                # (CNP / LNP: the launches of ``_context_stage`` with the per-point representations kept next to their mean, for
                # ``Conditioned.reweighted`` / ``kfold``)
                Xc_pt, R_pts = self._encode_points(X_cntxt, Y_cntxt)
                R = self._pool_pt(R_pts, B, n_valid=n_cntxt)
            else:
                Xc_pt, R = self._context_stage(X_cntxt, Y_cntxt, n_cntxt, fused_t)
            z_samples = q_zCc = None
            if n_z is not None:
                q_zCc = self._infer_q_zCc(R, B, n_cntxt if C > 0 else None)
                z_samples = q_zCc.rsample([n_z])
        return Conditioned(self, Xc_pt, R, z_samples, q_zCc, n_cntxt, B, C, fused_t, R_pts=R_pts)

    def condition_with_capacity(self, X_cntxt, Y_cntxt, capacity, n_cntxt=None, n_z_samples=None) -> "Conditioned":
        """:meth:`condition` into a context that can grow: the state is stored at ``capacity`` >= C rows per task (C = 0 is allowed)
        together with its own device counts (a copy of ``n_cntxt``, or C for every task), and :meth:`Conditioned.extend` /
        :meth:`Conditioned.rollout` add observations to it in place.  Such a model always runs the padded route of ``forward``
        (``n_cntxt``) with ``capacity`` key rows: masked attention / mean stop at the counts and never read the rows beyond.  Stored:
        the encoded context points and the per-point representations (every model: CNP / LNP re-pool their mean from the latter
        and decode ``Conditioned.loo`` at the former).  A latent model draws ``eps = randn([n_z, B, 1, z_dim])`` once -- the draw ``rsample`` makes in ``condition`` -- keeps
        it (``Conditioned.eps``) and sets ``z_samples = loc + scale * eps``, again after every ``extend``.  Not implemented, as with
        ``n_cntxt``: ``is_self_attn=True`` and the bf16 compute mode."""
        self._refuse_unimplemented("capacity")
        with torch.no_grad():
            n_z = self._n_z_for(n_z_samples)
            if X_cntxt.dim() != 3 or Y_cntxt.dim() != 3 or X_cntxt.shape[:2] != Y_cntxt.shape[:2]:
                raise ValueError(f"X_cntxt / Y_cntxt must be [B, C, x_dim] / [B, C, y_dim], got {list(X_cntxt.shape)} / {list(Y_cntxt.shape)}")
            B, C, _ = X_cntxt.shape
            capacity = int(capacity)
            if capacity < max(C, 1):
                raise ValueError(f"capacity={capacity} must be at least the context size C={C} (and at least 1)")
            self._check_tensors(X_cntxt, Y_cntxt)
            if n_cntxt is not None:
                n_cntxt = self._check_counts(n_cntxt, X_cntxt, "n_cntxt")
            if n_z is not None:
                self.n_z_samples = n_z
            dev = X_cntxt.device
            # (zeros: the rows beyond the counts are never read, but they stay finite for whoever looks at the state)
            R_pts = PTensor(torch.zeros(pt_shape(B, capacity, self.r_dim), device=dev), capacity, self.r_dim)
            # (the encoded points of every model: the keys of an attentive one, and the decoder's x of ``Conditioned.loo``)
            Xc_pt = PTensor(torch.zeros(pt_shape(B, capacity, self.x_transf_dim), device=dev), capacity, self.x_transf_dim)
            counts = torch.zeros(B, dtype=torch.int32, device=dev)
            post = Conditioned(self, Xc_pt, R_pts if self._attentive else torch.zeros(B, 1, self.r_dim, device=dev), None, None, counts,
                               B, C, False, capacity=capacity, R_pts=R_pts)
            if C > 0:
                Xn_pt, Rn_pts = self._encode_points(X_cntxt, Y_cntxt)
                pairs = [(Rn_pts.t, R_pts.t, self.r_dim), (Xn_pt.t, Xc_pt.t, self.x_transf_dim)]
                FN.append_points(pairs, counts, n_cntxt, B, C, capacity)
            post._refresh()
            if n_z is not None:
                post.q_zCc = q = self._infer_q_zCc(post._R, B, counts)
                post.eps = torch.randn(n_z, B, 1, self.z_dim, device=dev)
                post.z_samples = q.base_dist.loc + q.base_dist.scale * post.eps
        return post

    def loo(self, X_cntxt, Y_cntxt, n_cntxt=None) -> HeadDistribution:
        """The leave-one-out predictive of a context: for every task ``b`` and context point ``i``, p(y_i | the task's other points)
        at ``x_i`` -- what ``forward`` returns for the context cut to the other ``n - 1`` points with ``x_i`` as the only target -- out
        of ONE encode of the context.  Without a self-attention encoder the representation of a context point depends on that point
        alone, so this is exact: the attentive models run one masked attention launch whose queries are the encoded context points
        and in which query ``i`` does not see key ``i`` (``npf_masked_attn_fwd_loo``), CNP takes ``(sum - r_i) / (n - 1)``
        (``npf_loo_mean``); then the decoder and the masked head of the padded route.  -> :class:`HeadDistribution` with batch shape
        [1, B, C] and event shape [y_dim] whose target counts are the context counts: ``log_prob(Y_cntxt)`` is the per-point LOO log
        density, ``summary(probs)`` / ``base_dist`` work as on any other; rows at and beyond ``n_cntxt[b]`` (optional per-task sizes of
        a padded context, default C for every task) have ``loc = 0`` / ``scale = 1``, and a task with a single point is predicted from
        the empty context.  Inference only (``torch.no_grad`` semantics, the model's mode respected), no host sync and no range
        check: one captured graph serves every mix of counts.  Not implemented: ``is_self_attn=True``, the bf16 compute mode and the
        latent models (q(z | C without i) differs per left-out point, and the decoder takes one z per task)."""
        self._refuse_loo()
        if X_cntxt.dim() != 3 or Y_cntxt.dim() != 3 or X_cntxt.shape[:2] != Y_cntxt.shape[:2]:
            raise ValueError(f"X_cntxt / Y_cntxt must be [B, C, x_dim] / [B, C, y_dim], got {list(X_cntxt.shape)} / {list(Y_cntxt.shape)}")
        B, C, _ = X_cntxt.shape
        if C == 0:
            raise ValueError("loo: no context points")
        with torch.no_grad():
            if n_cntxt is not None:
                n_cntxt = self._check_counts(n_cntxt, X_cntxt, "n_cntxt")
            self._check_tensors(X_cntxt, Y_cntxt)
            if n_cntxt is None:
                n_cntxt = torch.full((B,), C, dtype=torch.int32, device=X_cntxt.device)
            Xc_pt, R_pts = self._encode_points(X_cntxt, Y_cntxt)
            return self._loo_from(Xc_pt, R_pts, n_cntxt, B, C)

    def _refuse_loo(self):
        if self.encoded_path != "deterministic":
            raise NotImplementedError("loo is not implemented for latent models (LNP / AttnLNP): q(z | C without i) differs per "
                                      "left-out point and the decoder takes one z per task")
        self._refuse_unimplemented("loo")

    def _loo_from(self, Xc_pt, R_pts, n, B, rows) -> HeadDistribution:
        """The leave-one-out predictive from the encoded context points and their per-point representations (PTensors of ``rows`` rows
        per task, ``n`` [B] device int32 of them real)."""
        return self._head(self._loo_suffstat(Xc_pt, R_pts, n, B, rows), None, B, rows, n_trgt=n)

    def kfold(self, X_cntxt, Y_cntxt, folds, k, n_cntxt=None) -> HeadDistribution:
        """The k-fold predictive of a context: for every task ``b`` and context point ``i``, p(y_i | the task's points whose fold id
        differs from ``folds[b, i]``) at ``x_i`` -- what ``forward`` returns for the context cut to the other folds with ``x_i`` as
        the only target -- out of ONE encode of the context.  ``folds``: integer device tensor [B, C] of fold ids in [0, k) (ids
        outside are clamped into it), ``k`` a host int >= 2; contiguous bands of ids give leave-a-band-out.  The k replicates
        ``W[f, b, i] = (folds[b, i] != f)`` run as one weighted attention launch over the context points as queries
        (``npf_masked_attn_fwd_weighted``; CNP: one ``npf_weighted_mean``), one device index op picks for point ``i`` the row of
        replicate ``folds[b, i]``, and the decoder runs once on the gathered [B, C] representations.  -> :class:`HeadDistribution`
        with batch shape [1, B, C] whose target counts are the context counts, as with :meth:`loo` (``kfold(...).score(Y_cntxt)``
        gives the k-fold scores); a point whose fold holds every point of its task is predicted from the empty context.  With
        ``folds[b, i] = i`` and ``k = C`` this is :meth:`loo`.  Inference only, no host sync.  Not implemented: ``is_self_attn=True``,
        the bf16 compute mode and the latent models."""
        self._refuse_kfold()
        if X_cntxt.dim() != 3 or Y_cntxt.dim() != 3 or X_cntxt.shape[:2] != Y_cntxt.shape[:2]:
            raise ValueError(f"X_cntxt / Y_cntxt must be [B, C, x_dim] / [B, C, y_dim], got {list(X_cntxt.shape)} / {list(Y_cntxt.shape)}")
        B, C, _ = X_cntxt.shape
        if C == 0:
            raise ValueError("kfold: no context points")
        k = _check_folds(folds, k, B, C)
        with torch.no_grad():
            if n_cntxt is not None:
                n_cntxt = self._check_counts(n_cntxt, X_cntxt, "n_cntxt")
            self._check_tensors(X_cntxt, Y_cntxt)
            if folds.device != X_cntxt.device:
                raise ValueError(f"folds lives on {folds.device}, the batch on {X_cntxt.device}")
            if n_cntxt is None:
                n_cntxt = torch.full((B,), C, dtype=torch.int32, device=X_cntxt.device)
            Xc_pt, R_pts = self._encode_points(X_cntxt, Y_cntxt)
            return self._kfold_from(Xc_pt, R_pts, n_cntxt, folds, k, B, C)

    def _refuse_kfold(self):
        if self.encoded_path != "deterministic":
            raise NotImplementedError("kfold is not implemented for latent models (LNP / AttnLNP): q(z | C without the fold) differs "
                                      "per fold and the decoder takes one z per task; use Conditioned.reweighted with the fold masks")
        self._refuse_unimplemented("kfold")

    def _kfold_from(self, Xc_pt, R_pts, n, folds, k, B, rows) -> HeadDistribution:
        """The k-fold predictive from the encoded context points and their per-point representations (PTensors of ``rows`` rows per
        task, ``n`` [B] device int32 of them real): the representation of point ``i`` is that of replicate ``folds[b, i]``."""
        own = folds.long().clamp(0, k - 1)
        R_g = self._kfold_rep(Xc_pt, R_pts, n, kfold_weights(own, k), own, k, B, rows)
        return self._head(self._decode_pointwise(R_g, Xc_pt.t, B, rows), None, B, rows, n_trgt=n)

    def _decode_pointwise(self, R_t, X1_pt, B, T):
        """The decoder on one representation per target (PT32 ``R_t`` [B, T, r]) as the padded route of the attentive models runs it."""
        from . import x6

        if x6.decoder_side_usable(self, T):
            return x6.decoder_side(self, R_t, X1_pt, T)
        ch = Chain(B, T, X1_pt.device, wg_per_task=True)
        ch.input_pt(R_t, self.r_dim)
        return self.decoder.finish_rows(ch, x1_pt=X1_pt)

    def _encode_points(self, X, Y):
        """The per-point stages of the context side on [B, N, .] points -> (encoded points, per-point representations), PTensors of
        N rows: the launches the padded route of ``_context_stage`` runs for a context of this size, without its pooling."""
        if self._fused_context_side(X.shape[1]):
            from . import x6

            return x6.context_side(self, X, Y)
        X_pt = self._xenc_pt(X)
        return X_pt, self._xyenc_pt(X_pt, Y, with_tr=False)

    def predict(self, X_cntxt, Y_cntxt, X_trgt, n_cntxt=None, n_trgt=None, n_z_samples=None, probs=(0.025, 0.5, 0.975)) -> Prediction:
        """``condition(X_cntxt, Y_cntxt, n_cntxt, n_z_samples).query(X_trgt, n_trgt).summary(probs)``: mean, standard deviation and
        quantiles of p(y | context) at ``X_trgt``."""
        probs = FN.check_probs(probs)
        return self.condition(X_cntxt, Y_cntxt, n_cntxt=n_cntxt, n_z_samples=n_z_samples).query(X_trgt, n_trgt=n_trgt).summary(probs)

    def _refuse_unimplemented(self, what):
        """What the padded path does not implement (``what``: the argument that asks for it)."""
        from . import chain as _chain

        if getattr(self, "is_self_attn", False):
            raise NotImplementedError(f"{what} is not implemented for self-attention context encoders (is_self_attn=True)")
        if _chain.COMPUTE_DTYPE != "fp32":
            raise NotImplementedError(f"{what} is not implemented in the bf16 compute mode (set_compute_dtype('bf16'))")

    def _refuse_weights(self):
        """What ``forward(w_cntxt=...)`` does not implement."""
        self._refuse_unimplemented("w_cntxt")
        if isinstance(self, LatentNeuralProcessFamily):
            raise NotImplementedError("w_cntxt is not implemented for the latent models (LNP / AttnLNP): q(z | C, T) would need a rule "
                                      "for the weights of the targets")

    def _check_weights(self, w, X):
        """The context weights of the batch ``X`` [B, C, .] as the fp32 device tensor [B, C] the kernels read, still in the autograd
        graph; refuses what the weighted route does not implement.  The values are not looked at."""
        self._refuse_weights()
        B, C = X.shape[0], X.shape[1]
        if not isinstance(w, torch.Tensor) or not w.is_floating_point():
            raise ValueError(f"w_cntxt must be a float device tensor of shape [{B}, {C}], got "
                             f"{w.dtype if isinstance(w, torch.Tensor) else type(w).__name__}")
        if tuple(w.shape) != (B, C):
            raise ValueError(f"w_cntxt must have shape [{B}, {C}] (one weight per context point), got {list(w.shape)}")
        if w.device != X.device:
            raise ValueError(f"w_cntxt lives on {w.device}, the batch on {X.device}")
        return w.to(torch.float32).contiguous()

    def _check_counts(self, n, X, what):
        """The per-task sizes ``what`` (``n_cntxt`` / ``n_trgt``) of the padded batch ``X`` as a device int32 [B] tensor; refuses what
        the padded path does not implement."""
        self._refuse_unimplemented(what)
        n = FN.counts_i32(n, X.shape[0], what)
        if n.device != X.device:
            raise ValueError(f"{what} lives on {n.device}, the batch on {X.device}")
        return n

    def _validate_inputs(self, X_cntxt, Y_cntxt, X_trgt, Y_trgt):
        """base.py:241-247: features must be in [-1, 1] during training (the padding rows of a padded batch included)."""
        self._check_tensors(X_cntxt, Y_cntxt, X_trgt, Y_trgt)
        if self.training and self.validate_inputs:
            # one device reduction and ONE host sync per step (every sync drains the stream and
            # costs a launch bubble); NaNs fail the test like the reference's (x>=-1)&(x<=1)
            m = X_trgt.abs().amax() if X_trgt.numel() else X_trgt.new_zeros(())
            if X_cntxt.numel():
                m = torch.maximum(m, X_cntxt.abs().amax())
            if self.validate_inputs == "deferred":
                # (a step replayed from a HIP graph cannot stop for the host: the reduction stays in the step, the
                # running maximum -- NaN-propagating -- is read by ``check_deferred_inputs`` at the next sync point)
                if getattr(self, "_range_seen", None) is None or self._range_seen.device != m.device:
                    self._range_seen = torch.zeros((), device=m.device)
                self._range_seen.copy_(torch.maximum(self._range_seen, m))
                return
            if not (m.item() <= 1.0):
                lo = min(X_cntxt.min().item() if X_cntxt.numel() else 0.0, X_trgt.min().item())
                hi = max(X_cntxt.max().item() if X_cntxt.numel() else 0.0, X_trgt.max().item())
                raise ValueError(f"Features during training should be in [-1,1]. Got [{lo}, {hi}].")

    @staticmethod
    def _check_tensors(*tensors):
        for t in tensors:
            if t is not None and (not t.is_cuda or t.dtype != torch.float32):
                raise RuntimeError("the HIP path takes fp32 device tensors only; there is no CPU fallback")

    def check_deferred_inputs(self):
        """``validate_inputs == "deferred"``: raise the reference's ValueError (base.py:244-247) if any training batch
        since the last call had features outside [-1, 1] (one host sync, resets the record)."""
        seen = getattr(self, "_range_seen", None)
        if seen is None:
            return
        worst = seen.item()
        seen.zero_()
        if not (worst <= 1.0):
            raise ValueError(f"Features during training should be in [-1,1]. Got max |x| = {worst}.")

    # ------------------------------------------------------------------ PT-level stages
    _attentive = False  # attentive subclasses also keep feature-major copies of keys / values

    def _fused_target_side(self, C, T) -> bool:
        """Does ``forward`` hand the whole target side (x-encoder, attention, decoder) to one x6 program (x6.py)."""
        return False

    def _xenc_with_query_projection(self, C, T) -> bool:
        """Does ``forward`` hand the target x-encoder + the attender's query projection to one x6 program (x6.xenc_proj)."""
        from . import x6

        att = getattr(self, "attender", None)
        if not (self._attentive and isinstance(att, MultiheadAttender) and C > 0):
            return False
        return FN.mha_usable(att.kq_head_size, att.value_head_size, C) and x6.xenc_proj_usable(self, att.query_transform, T)

    def _fused_context_side(self, C) -> bool:
        """Does ``forward`` hand x-encoder + XY-encoder of the context points to one x6 program (x6.py)."""
        from . import x6

        return hasattr(self, "xy_encoder") and hasattr(self, "_pool_pt") and x6.context_side_usable(self, C)

    def _xenc_pt(self, X, with_tr=False) -> PTensor:
        B, P, dx = X.shape
        ch = Chain(B, P, X.device)
        ch.input_rows(X.contiguous(), dx)
        return self.x_encoder.append_to(ch).run_pt(as_weights=with_tr)

    def _xyenc_pt(self, X_enc: PTensor, Y, with_tr: Optional[bool] = None) -> PTensor:
        """Per-point XY encoding (the per-point part of encode_globally) -> [B, P, r]."""
        ch = Chain(X_enc.n_tasks, X_enc.pts, Y.device)
        ch.input_rows(Y.contiguous(), self.y_dim)
        return self.xy_encoder.run_pt(ch, X_enc.t, X_enc.n_tasks, X_enc.pts,
                                      with_tr=self._attentive if with_tr is None else with_tr)

    def _head(self, suff, Y_trgt, B, T, n_trgt=None):
        return HeadDistribution(suff, self.y_dim, not self.is_heteroskedastic, suff.shape[0] // B, B, T, n_trgt=n_trgt)

    def _decode_taskvec(self, Xt_pt, vec, B, T, n_rows):
        """decoder(X_trgt_enc, R_trgt) when R_trgt is one vector per (z-sample, task)
        (np.py:107-110,161: the reference expands it over the targets and recomputes the
        resizer per target; here the resizer runs once per task)."""
        ch = Chain(n_rows, T, Xt_pt.t.device)
        ch.input_pt(Xt_pt.t, self.x_transf_dim, modulus=(B if n_rows != B else 0))
        return self.decoder.finish_rows(ch, taskvec=vec)

    # ------------------------------------------------------------------ reference stage API (row-major)
    @abc.abstractmethod
    def encode_globally(self, X_cntxt, Y_cntxt):
        pass

    @abc.abstractmethod
    def trgt_dependent_representation(self, X_cntxt, z_samples, R, X_trgt):
        pass

    def latent_path(self, X_cntxt, R, X_trgt, Y_trgt):
        raise NotImplementedError(
            f"`latent_path` not implemented. Cannot use encoded_path={self.encoded_path} in such case.")

    def decode(self, X_trgt, R_trgt):
        """base.py:327-367 with row-major ``X_trgt`` [B,T,x_transf] and ``R_trgt`` [n_z,B,T,r]."""
        n_z, B, T, _ = R_trgt.shape
        suff = self.decoder(X_trgt, R_trgt).reshape(n_z * B, T, 2 * self.y_dim)
        return self._head(suff, None, B, T)

    def set_extrapolation(self, min_max):
        pass


class LatentNeuralProcessFamily(NeuralProcessFamily):
    """Latent (sub-)family (npf/neuralproc/base.py:374-575)."""

    _valid_paths = ["latent", "both"]

    def __init__(self, *args, is_q_zCct=False, n_z_samples_train=32, n_z_samples_test=32, LatentEncoder=None,
                 LatentDistribution=MultivariateNormalDiag, q_z_loc_transformer=None, q_z_scale_transformer=None,
                 z_dim=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.is_q_zCct = is_q_zCct
        self.n_z_samples_train, self.n_z_samples_test = n_z_samples_train, n_z_samples_test
        self.z_dim = self.r_dim if z_dim is None else z_dim
        if LatentEncoder is None:
            LatentEncoder = self.dflt_Modules["LatentEncoder"]
        self.latent_encoder = LatentEncoder(self.r_dim, self.z_dim * 2)
        if self.encoded_path == "both":
            self.r_z_merger = nn.Linear(self.r_dim + self.z_dim, self.r_dim)
        self.LatentDistribution = LatentDistribution
        self.q_z_loc_transformer = nn.Identity() if q_z_loc_transformer is None else q_z_loc_transformer
        self.q_z_scale_transformer = _q_z_scale if q_z_scale_transformer is None else q_z_scale_transformer
        if self.z_dim != self.r_dim and self.encoded_path == "latent":
            self.reshaper_z = nn.Linear(self.z_dim, self.r_dim)

    @property
    def dflt_Modules(self):
        d = NeuralProcessFamily.dflt_Modules.__get__(self)
        d["LatentEncoder"] = partial(MLP, n_hidden_layers=1, hidden_size=self.r_dim)
        return d

    def forward(self, *args, **kwargs):
        self.n_z_samples = self._n_z_for()
        return super().forward(*args, **kwargs)

    def _n_z_for(self, n_z_samples=None) -> int:
        if n_z_samples is not None:
            if int(n_z_samples) < 1:
                raise ValueError(f"n_z_samples must be at least 1, got {n_z_samples}")
            return int(n_z_samples)
        try:  # scipy random variable = random number of samples (base.py:478-486)
            return self.n_z_samples_train.rvs() if self.training else self.n_z_samples_test.rvs()
        except AttributeError:
            return self.n_z_samples_train if self.training else self.n_z_samples_test

    def infer_latent_dist(self, X, R):
        """base.py:516-547 on row-major R."""
        R_lat_inp = self.rep_to_lat_input(R)
        return self._latent_dist_from(R_lat_inp)

    def _latent_dist_from(self, R_lat_inp):
        suff = self.latent_encoder(R_lat_inp)
        q_z_loc, q_z_scale = suff.split(self.z_dim, dim=-1)
        return self.LatentDistribution(self.q_z_loc_transformer(q_z_loc), self.q_z_scale_transformer(q_z_scale))

    def rep_to_lat_input(self, R):
        return R

    def latent_path(self, X_cntxt, R, X_trgt, Y_trgt):
        """base.py:495-514 (row-major stage API)."""
        q_zCc = self.infer_latent_dist(X_cntxt, R)
        if self.is_q_zCct and Y_trgt is not None:
            R_from_trgt = self.encode_globally(X_trgt, Y_trgt)
            q_zCct = self.infer_latent_dist(X_trgt, R_from_trgt)
            sampling_dist = q_zCct
        else:
            q_zCct, sampling_dist = None, q_zCc
        return sampling_dist.rsample([self.n_z_samples]), q_zCc, q_zCct

    def _infer_q_zCc(self, R, B, n_valid=None):
        """q(z | C) from the context representation (``n_valid``: the context sizes of a padded batch)."""
        return self._latent_dist_from(self._lat_input(R, B, n_valid=n_valid))

    def _latent_path_pt(self, R, C, Xt_pt, Y_trgt, B, T, n_valid=None, n_trgt=None):
        # (n_valid: the context sizes of a padded batch; n_trgt: the target sizes -- the target-side encode below pools over the
        # first n_trgt[b] targets, zeros for a task without any, as encode_globally at zero points)
        q_zCc = self._infer_q_zCc(R, B, n_valid)
        if self.is_q_zCct and Y_trgt is not None:
            if Xt_pt is None:
                # (forward left the target side to one x6 program, which encodes the targets itself: the target-side latent
                # encode of base.py:501-506 is the context-side program over the target points, or the chain launches)
                if self._fused_context_side(T):
                    from . import x6

                    R_t = self._pool_pt(x6.context_side(self, self._X_trgt_raw, Y_trgt)[1], B, n_valid=n_trgt)
                else:
                    R_t = self._encode_globally_pt(self._xenc_pt(self._X_trgt_raw), Y_trgt, B, T, n_valid=n_trgt)
            else:
                R_t = self._encode_globally_pt(Xt_pt, Y_trgt, B, T, n_valid=n_trgt)
            q_zCct = self._latent_dist_from(self._lat_input(R_t, B, n_valid=n_trgt))
            sampling_dist = q_zCct
        else:
            q_zCct, sampling_dist = None, q_zCc
        return sampling_dist.rsample([self.n_z_samples]), q_zCc, q_zCct

    def merge_r_z(self, R, z_samples):
        """base.py:554-575 on row-major tensors: relu(Linear(cat(R, z)))."""
        if R.shape != z_samples.shape:
            R = R.unsqueeze(0).expand(*z_samples.shape[:-1], self.r_dim)
        lead = z_samples.shape[:-1]
        rows = int(math.prod(lead))
        out = self._merge_rows(R.reshape(rows, self.r_dim), z_samples.reshape(rows, self.z_dim))
        return out.reshape(*lead, self.r_dim)

    def _merge_rows(self, R_rows, z_rows):
        """relu(W_R R + (W_z z + b)) on [rows, .] tensors; the concatenation of the reference
        is never materialised (two accumulating layers)."""
        rows = R_rows.shape[0]
        W, b, r = self.r_z_merger.weight, self.r_z_merger.bias, self.r_dim
        ch = Chain(1, rows, R_rows.device)
        ch.input_pt(FN.pack_pt(z_rows.reshape(1, rows, self.z_dim)), self.z_dim).linear(W[:, r:], b).output_pt()
        (zb,) = ch.run()
        ch = Chain(1, rows, R_rows.device)
        ch.input_pt(FN.pack_pt(R_rows.reshape(1, rows, r)), r).linear(W[:, :r], None, relu=True, addend=zb).output_pt()
        return FN.unpack_pt(ch.run()[0], rows, r).reshape(rows, r)


class CNP(NeuralProcessFamily):
    """Conditional neural process: mean aggregation (npf/neuralproc/np.py:19-110)."""

    _valid_paths = ["deterministic"]

    def __init__(self, x_dim, y_dim, XYEncoder=None, **kwargs):
        kwargs["encoded_path"] = kwargs.get("encoded_path", "deterministic")
        super().__init__(x_dim, y_dim, **kwargs)
        if XYEncoder is None:
            XYEncoder = self.dflt_Modules["XYEncoder"]
        self.xy_encoder = XYEncoder(self.x_transf_dim, self.y_dim, self.r_dim)
        if not isinstance(self.xy_encoder, MergeFlatInputs):
            raise NotImplementedError("the HIP path needs the stock merge_flat_input(MLP) XYEncoder")

    @property
    def dflt_Modules(self):
        d = NeuralProcessFamily.dflt_Modules.__get__(self)
        sub = partial(MLP, n_hidden_layers=2, is_force_hid_smaller=True, hidden_size=self.r_dim)
        d["XYEncoder"] = merge_flat_input(sub, is_sum_merge=True)
        return d

    forward = NeuralProcessFamily._forward_weighted  # (forward(..., n_cntxt=None, n_trgt=None, w_cntxt=None))

    # reference stage API
    def encode_globally(self, X_cntxt, Y_cntxt):
        B, C, _ = X_cntxt.shape
        if C == 0:
            return torch.zeros(B, 1, self.r_dim, device=X_cntxt.device)
        return self._encode_globally_pt(PTensor(FN.pack_pt(X_cntxt), C, self.x_transf_dim), Y_cntxt, B, C)

    def trgt_dependent_representation(self, _, __, R, X_trgt):
        B, T, _ = X_trgt.shape
        return R.expand(B, T, self.r_dim).unsqueeze(0)

    # fused path
    def _encode_globally_pt(self, X_enc, Y, B, P, n_valid=None):
        """-> row-major R [B, 1, r] (np.py:86-101)."""
        if P == 0:
            return torch.zeros(B, 1, self.r_dim, device=Y.device)
        return self._pool_pt(self._xyenc_pt(X_enc, Y), B, n_valid=n_valid)

    def _pool_pt(self, R_pts: PTensor, B, n_valid=None):
        """np.py:95: the mean over the context points of the per-point representations -> row-major [B, 1, r]; ``n_valid``: over
        the first ``n_valid[b]`` of them (a padded batch; zeros for a task without context, as ``encode_globally`` at C = 0)."""
        return _mean_rows(R_pts.t, R_pts.pts, B, self.r_dim, n_valid)

    def _target_suffstat(self, Xc_pt, z_samples, R, Xt_pt, B, C, T, n_valid=None, n_q_valid=None):
        return self._decode_taskvec(Xt_pt, R.reshape(B, self.r_dim), B, T, B)

    def _loo_suffstat(self, Xc_pt, R_pts, n, B, rows):
        """Point ``i`` is decoded at ``x_i`` from the mean over the task's other points (zeros where there is none, as
        ``encode_globally`` at C = 0)."""
        return self._decode_pointwise(FN.loo_mean(R_pts.t, n, B, rows, self.r_dim), Xc_pt.t, B, rows)

    def _kfold_rep(self, Xc_pt, R_pts, n, W, own, k, B, rows):
        """PT32 [B, rows, r]: row ``i`` is the mean over the task's points outside fold ``own[b, i]`` -- the k weighted means per
        task, then one index op (zeros where no point is left, as ``encode_globally`` at C = 0)."""
        r = self.r_dim
        means = FN.weighted_mean(R_pts.t, W, n, k * B, B, rows, r)[:, :r].view(k, B, r)
        return FN.pack_pt(means[own, torch.arange(B, device=own.device).view(B, 1)])


class LNP(LatentNeuralProcessFamily, CNP):
    """(Latent) neural process (npf/neuralproc/np.py:113-163)."""

    _valid_paths = ["latent", "both"]

    def __init__(self, x_dim, y_dim, encoded_path="latent", **kwargs):
        super().__init__(x_dim, y_dim, encoded_path=encoded_path, **kwargs)

    def _lat_input(self, R, B, n_valid=None):
        return R

    def _rep_rows(self, z_samples, R, B):
        n_z = z_samples.size(0)
        if self.encoded_path == "both":
            R_trgt = self.merge_r_z(R, z_samples)
        else:
            R_trgt = z_samples
            if self.z_dim != self.r_dim:
                R_trgt = _rows_mlp_linear(self.reshaper_z, R_trgt)
        return R_trgt.reshape(n_z * B, self.r_dim)

    def trgt_dependent_representation(self, _, z_samples, R, X_trgt):
        B, T, _ = X_trgt.shape
        n_z = z_samples.size(0)
        return self._rep_rows(z_samples, R, B).reshape(n_z, B, 1, self.r_dim).expand(n_z, B, T, self.r_dim)

    def _target_suffstat(self, Xc_pt, z_samples, R, Xt_pt, B, C, T, n_valid=None, n_q_valid=None):
        n_z = z_samples.size(0)
        return self._decode_taskvec(Xt_pt, self._rep_rows(z_samples, R, B), B, T, n_z * B)


def _rows_mlp_linear(lin: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    lead = x.shape[:-1]
    rows = int(math.prod(lead))
    ch = Chain(1, rows, x.device)
    ch.input_pt(FN.pack_pt(x.reshape(1, rows, x.shape[-1])), x.shape[-1]).linear(lin.weight, lin.bias).output_pt()
    return FN.unpack_pt(ch.run()[0], rows, lin.out_features).reshape(*lead, lin.out_features)


class AttnCNP(NeuralProcessFamily):
    """Attentive conditional neural process (npf/neuralproc/attnnp.py:27-131)."""

    _valid_paths = ["deterministic"]
    _attentive = True

    def __init__(self, x_dim, y_dim, XYEncoder=None, attention="scaledot", attention_kwargs={},
                 self_attention_kwargs={}, is_self_attn=False, **kwargs):
        kwargs["encoded_path"] = kwargs.get("encoded_path", "deterministic")
        super().__init__(x_dim, y_dim, **kwargs)
        self.is_self_attn = is_self_attn
        if is_self_attn:
            # attnnp.py:88-91: relu(x + resizer(y)) followed by self-attention layers over the context
            XYEncoder = merge_flat_input(SelfAttention, is_sum_merge=True, **self_attention_kwargs)
        elif XYEncoder is None:
            XYEncoder = self.dflt_Modules["XYEncoder"]
        self.xy_encoder = XYEncoder(self.x_transf_dim, self.y_dim, self.r_dim)
        if not isinstance(self.xy_encoder, MergeFlatInputs):
            raise NotImplementedError("the HIP path needs the stock merge_flat_input(MLP) XYEncoder")
        self.attender = get_attender(attention, self.x_transf_dim, self.r_dim, self.r_dim, **attention_kwargs)
        if not isinstance(self.attender, (DotAttender, MultiheadAttender)):
            raise NotImplementedError("the HIP path implements attention = 'scaledot', 'multihead', 'transformer'")

    dflt_Modules = CNP.dflt_Modules
    forward = NeuralProcessFamily._forward_weighted  # (forward(..., n_cntxt=None, n_trgt=None, w_cntxt=None))

    def _fused_target_side(self, C, T) -> bool:
        from . import x6

        return type(self) is AttnCNP and self.encoded_path == "deterministic" and x6.target_side_usable(self, C, T)

    # reference stage API
    def encode_globally(self, X_cntxt, Y_cntxt):
        B, C, _ = X_cntxt.shape
        if C == 0:
            return torch.zeros(B, 0, self.r_dim, device=X_cntxt.device)
        return self.xy_encoder(X_cntxt, Y_cntxt)

    def trgt_dependent_representation(self, X_cntxt, _, R, X_trgt):
        B, C, _ = X_cntxt.shape
        if C == 0:
            R_trgt = torch.zeros(B, X_trgt.size(1), self.r_dim, device=R.device)
        else:
            R_trgt = self.attender(X_cntxt, X_trgt, R)
        return R_trgt.unsqueeze(0)

    # fused path
    def _encode_globally_pt(self, X_enc, Y, B, P, n_valid=None):
        """-> R_cntxt [B, P, r] as a PTensor (attnnp.py:105-116); None when there is no context."""
        if P == 0:
            return None
        # (a padded batch attends on the masked kernel, which reads the PT32 tensors: no feature-major copies)
        return self._xyenc_pt(X_enc, Y, with_tr=None if n_valid is None else False)

    def _pool_pt(self, R_pts: PTensor, B, n_valid=None):
        """attnnp.py:105-116: no pooling, one representation per context point."""
        return R_pts

    def _attend_padded(self, Xc_pt, R, Xt_pt, B, C, T, n_valid, n_q_valid=None):
        """PT32 [B, T, r]: attention of the targets over the first ``n_valid[b]`` context points of every task (attnnp.py:118-131
        on the batch cut per task).  A task without context gets zeros, as ``trgt_dependent_representation`` at C = 0 -- also
        behind an attender whose learned layers would turn zero context vectors into something else.  ``n_q_valid``: the target
        sizes of a batch whose targets are padded too; the attention skips the queries beyond them."""
        k_pt, v_pt = (None, None) if Xc_pt is None else (Xc_pt.t, R.t)  # (a PrefixTail carries its own keys / values)
        R_t = self.attender.attend_pt(Xt_pt.t, k_pt, v_pt, C, T, n_valid=n_valid, n_q_valid=n_q_valid)
        live = as_key_rule(n_valid).live(B)
        if not isinstance(self.attender, DotAttender):
            R_t = R_t * live.to(R_t.dtype).view(B, 1, 1, 1, 1)
        return R_t

    def _loo_suffstat(self, Xc_pt, R_pts, n, B, rows):
        """The padded route with the encoded context points as targets and the diagonal of the attention excluded."""
        return self._target_suffstat(Xc_pt, None, R_pts, Xc_pt, B, rows, rows, n_valid=LeaveOneOut(n), n_q_valid=n)

    def _kfold_rep(self, Xc_pt, R_pts, n, W, own, k, B, rows):
        """PT32 [B, rows, r]: row ``i`` is the attention of context point ``i`` over the task's points outside fold ``own[b, i]`` --
        the padded route over k * B replicate tasks with the encoded context points as queries, then one index op over the
        replicates (whole PT32 tiles: the rows beyond ``rows`` take replicate 0's zeros)."""
        Xq = PTensor(Xc_pt.t.repeat(k, 1, 1, 1, 1), rows, self.x_transf_dim)
        R_t = self._attend_padded(Xc_pt, R_pts, Xq, k * B, rows, rows, KeyWeights(W, n, k), n_q_valid=n.repeat(k))
        tiles = R_t.shape[1]
        idx = torch.zeros(B, tiles * 32, dtype=torch.long, device=own.device)
        idx[:, :rows] = own
        idx = idx.view(1, B, tiles, 1, 32, 1).expand(1, B, tiles, R_t.shape[2], 32, 4)
        return torch.gather(R_t.view(k, B, *R_t.shape[1:]), 0, idx)[0]

    def _attend_into(self, ch, Xc_pt, R, Xt_pt, C, T, tap_x1: bool = False):
        """cur of ``ch`` <- attention of the targets over the context (attnnp.py:118-131): fused into
        the chain while a score row fits the registers, blocked (attention_long.py) beyond that."""
        from . import chain as _chain

        if not isinstance(self.attender, DotAttender):  # learned projections: its own launches
            ch.input_pt(self.attender.attend_pt(Xt_pt.t, Xc_pt.t, R.t, C, T, queries_proj=Xt_pt.proj), self.r_dim)
        elif _chain.COMPUTE_DTYPE == "bf16":
            if Xc_pt.img is not None and R.img is not None and self.attender.fits_fused(C):
                # bf16 compute mode with bf16 images of keys / values: attention and decoder in one bf16 chain
                ch.input_pt(Xt_pt.t, self.x_transf_dim)
                self.attender.append_to(ch, Xc_pt.t, R.t, C, keys_tr=Xc_pt.tr, values_tr=R.tr, keys_img=Xc_pt.img,
                                        values_img=R.img)
            else:  # the attention keeps an fp32 launch, the decoder chain behind it is bf16
                ch.input_pt(self.attender.attend_pt(Xt_pt.t, Xc_pt.t, R.t, C, T, keys_tr=Xc_pt.tr, values_tr=R.tr), self.r_dim)
        elif self.attender.fits_fused(C):
            ch.input_pt(Xt_pt.t, self.x_transf_dim)
            if tap_x1:
                # the encoded targets are the attention's queries here and the decoder's x1 on the split kernel next: handed on
                # through this chain, both gradients meet in its dgrad launch (MergeFlatInputs.finish_rows)
                ch.tap(alias_input=True)
                ch.x1_tapped = True
            self.attender.append_to(ch, Xc_pt.t, R.t, C, keys_tr=Xc_pt.tr, values_tr=R.tr)
        else:
            ch.input_pt(self.attender.attend_pt(Xt_pt.t, Xc_pt.t, R.t, C, T, keys_tr=Xc_pt.tr, values_tr=R.tr), self.r_dim)
        return ch

    def _target_suffstat(self, Xc_pt, z_samples, R, Xt_pt, B, C, T, n_valid=None, n_q_valid=None):
        if n_valid is not None:  # (a padded batch: masked attention, then the decoder as an unfused step runs it)
            from . import x6

            R_t = self._attend_padded(Xc_pt, R, Xt_pt, B, C, T, n_valid, n_q_valid)
            if x6.decoder_side_usable(self, T):
                return x6.decoder_side(self, R_t, Xt_pt.t, T)
            ch = Chain(B, T, Xt_pt.t.device, wg_per_task=True)
            ch.input_pt(R_t, self.r_dim)
            return self.decoder.finish_rows(ch, x1_pt=Xt_pt.t)
        if Xt_pt is None:  # (forward left the target side to the fused x6 program: x-encoder, attention, decoder in one launch)
            from . import x6

            return x6.target_side(self, self._X_trgt_raw, Xc_pt, R)
        if C > 0 and not isinstance(self.attender, DotAttender):
            from . import x6

            if x6.decoder_side_usable(self, T):
                # learned projections (multihead / transformer attention): its own launches, then the decoder as one x6 program
                return x6.decoder_side(self, self.attender.attend_pt(Xt_pt.t, Xc_pt.t, R.t, C, T, queries_proj=Xt_pt.proj), Xt_pt.t, T)
        ch = Chain(B, T, Xt_pt.t.device, wg_per_task=True)
        if C == 0:
            ch.input_pt(torch.zeros(pt_shape(B, T, self.r_dim), device=Xt_pt.t.device), self.r_dim)
        else:
            self._attend_into(ch, Xc_pt, R, Xt_pt, C, T, tap_x1=self.decoder.x6_resizer_ok())
        return self.decoder.finish_rows(ch, x1_pt=Xt_pt.t)


class AttnLNP(LatentNeuralProcessFamily, AttnCNP):
    """Attentive latent neural process: deterministic attention path + mean-pooled latent
    path, merged per target (npf/neuralproc/attnnp.py:134-202)."""

    _valid_paths = ["both"]

    def __init__(self, x_dim, y_dim, **kwargs):
        super().__init__(x_dim, y_dim, encoded_path="both", **kwargs)

    @property
    def dflt_Modules(self):
        d = AttnCNP.dflt_Modules.__get__(self)
        d.update(LatentNeuralProcessFamily.dflt_Modules.__get__(self))
        return d

    def rep_to_lat_input(self, R):
        B, C, _ = R.shape
        if C == 0:
            return torch.zeros(B, 1, self.r_dim, device=R.device)
        return _mean_rows(FN.pack_pt(R), C, B, self.r_dim)

    def _lat_input(self, R: Optional[PTensor], B, n_valid=None):
        """attnnp.py:172-181: the latent path pools the per-point representation (its own point count; ``n_valid``: the first
        ``n_valid[b]`` points of a padded batch)."""
        if R is None:
            return torch.zeros(B, 1, self.r_dim, device=self.r_z_merger.weight.device)
        return _mean_rows(R.t, R.pts, B, self.r_dim, n_valid)

    def trgt_dependent_representation(self, X_cntxt, z_samples, R, X_trgt):
        B, T, _ = X_trgt.shape
        n_z = z_samples.size(0)
        z = z_samples.expand(n_z, B, T, self.z_dim)
        R_det = AttnCNP.trgt_dependent_representation(self, X_cntxt, None, R, X_trgt).squeeze(0)
        return self.merge_r_z(R_det, z)

    def _fused_target_side(self, C, T) -> bool:
        """One latent sample, scaled-dot attention over <= 256 context points, 256-wide layers: the whole target side --
        x-encoder, attention, merge_r_z, decoder -- is one x6 program (x6.target_side with the latent merge)."""
        from . import x6

        return (type(self) is AttnLNP and self.n_z_samples == 1 and self.z_dim == self.r_dim
                and x6.target_side_usable(self, C, T, latent_merge=True))

    def _target_suffstat(self, Xc_pt, z_samples, R, Xt_pt, B, C, T, n_valid=None, n_q_valid=None):
        n_z = z_samples.size(0)
        dev = z_samples.device
        W, b, r = self.r_z_merger.weight, self.r_z_merger.bias, self.r_dim
        # the latent half of merge_r_z is constant per (z-sample, task): a per-task bias
        rows = n_z * B
        chz = Chain(1, rows, dev)
        chz.input_pt(FN.pack_pt(z_samples.reshape(1, rows, self.z_dim)), self.z_dim).linear(W[:, r:], b).output_pt()
        zb = FN.unpack_pt(chz.run()[0], rows, pad32(r)).reshape(rows, pad32(r))
        if Xt_pt is None:  # (the fused target side: one launch forward, one for its dgrad)
            from . import x6

            return x6.target_side(self, self._X_trgt_raw, Xc_pt, R, zb=zb)
        R_pad = self._attend_padded(Xc_pt, R, Xt_pt, B, C, T, n_valid, n_q_valid) if n_valid is not None else None
        if n_z == 1 and C > 0 and (R_pad is not None or not isinstance(self.attender, DotAttender)) and self.z_dim == self.r_dim:
            from . import x6

            if x6.decoder_side_usable(self, T):  # (attention with learned projections, then merge_r_z + decoder as one program)
                R_t = R_pad if R_pad is not None else self.attender.attend_pt(Xt_pt.t, Xc_pt.t, R.t, C, T, queries_proj=Xt_pt.proj)
                return x6.decoder_side(self, R_t, Xt_pt.t, T, zb=zb[:, :r].contiguous())
        if n_z == 1:
            ch = Chain(B, T, dev, wg_per_task=True)
            if C == 0:
                ch.input_pt(torch.zeros(pt_shape(B, T, r), device=dev), r)
            elif R_pad is not None:
                ch.input_pt(R_pad, r)
            else:
                self._attend_into(ch, Xc_pt, R, Xt_pt, C, T)
            mod = 0
        else:
            if C == 0:
                R_det = torch.zeros(pt_shape(B, T, r), device=dev)
            elif R_pad is not None:
                R_det = R_pad
            else:
                cha = Chain(B, T, dev, wg_per_task=True)
                self._attend_into(cha, Xc_pt, R, Xt_pt, C, T).output_pt()
                (R_det,) = cha.run()
            ch = Chain(rows, T, dev, wg_per_task=True)
            ch.input_pt(R_det, r, modulus=B)
            mod = B
        ch.linear(W[:, :r], zb, relu=True, bias_per_task=True)
        return self.decoder.finish_rows(ch, x1_pt=Xt_pt.t, x1_modulus=mod)
