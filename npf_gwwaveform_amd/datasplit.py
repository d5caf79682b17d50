"""Context / target split on the device: the step right before the path.

Mirrors, for 1-D / set-structured data, the reference's ``npf/utils/datasplit.py``:
``get_all_indcs`` (:30-34), ``GetRangeIndcs`` (:37-45), ``GetRandomIndcs`` (:60-145) and
``CntxtTrgtGetter`` (:148-255), with the same constructor arguments and call signatures.  The
reference samples indices with numpy on the host (one ``np.random.shuffle`` per batch row) and
gathers on whatever device ``X`` lives; here the per-row random subsets are drawn on the device
(argsort of uniform noise: every row an independent uniformly random subset, same distribution,
no host round trip) and the gather is one HIP launch for X and y together
(``npf_gather_points``).  Explicit ``context_indcs`` / ``target_indcs`` give bit-identical
selections to the reference's ``torch.gather``.  The *number* of points is a host-side draw
(``random.randint`` / ``scipy.stats.betabinom``), as in the reference.  The grid / mask getters
(images) are out of scope.
"""
from __future__ import annotations

import random
from typing import Optional

import numpy as np
import torch

from . import _lib as L

__all__ = ["get_all_indcs", "GetRangeIndcs", "GetRandomIndcs", "CntxtTrgtGetter"]


def _point_count(spec, n_points: int) -> int:
    """A number of points given either as a count (1 <= spec <= n_points) or as a fraction of ``n_points``
    (0 <= spec < 1), the convention of the reference's getters (npf/utils/helpers.py:99-108)."""
    if 0 <= spec < 1:
        return int(spec * n_points)
    if 1 <= spec <= n_points:
        return int(spec)
    raise ValueError("percentage={} outside of [0,{}].".format(spec, n_points))


def get_all_indcs(batch_size, n_possible_points, device=None):
    """All indices for every batch element (datasplit.py:30-34)."""
    return torch.arange(n_possible_points, device=device).expand(batch_size, n_possible_points)


class GetRangeIndcs:
    """All indices in a range (datasplit.py:37-45)."""

    def __init__(self, arange):
        self.arange = arange

    def __call__(self, batch_size, n_possible_points, device=None):
        indcs = torch.arange(*self.arange, device=device)
        return indcs.expand(batch_size, len(indcs))


class GetRandomIndcs:
    """Random subset of indices (datasplit.py:60-145), drawn on ``device``.

    ``is_per_task=True`` (no reference counterpart; the reference draws one size per batch): one count PER TASK between the
    same ``a`` and ``b``, drawn on the device with the same ``torch.Generator`` as the indices (no host sync, Python's
    ``random`` is not touched).  The indices come back padded to the largest possible count ``_point_count(b, n)`` -- a
    shape that does not change from batch to batch, which is what a captured graph needs -- and the counts of the last
    draw are in ``last_counts`` (int64 [batch_size]): row ``i`` uses its first ``last_counts[i]`` indices, the model takes
    the counts as ``n_cntxt`` (``n_trgt`` when it is the targets getter).  The default keeps the reference's behaviour.

    ``n_points`` (call argument, with ``is_per_task=True`` only): an integer device tensor [batch_size] for a padded DATA SET --
    row ``i`` has ``n_points[i]`` real points out of ``n_possible_points``.  Its indices are drawn among its first
    ``n_points[i]`` points only and its count is clamped to ``n_points[i]``; all on the device, no host sync."""

    def __init__(self, a=0.1, b=0.5, is_batch_share=False, range_indcs=None, is_ensure_one=False,
                 is_beta_binomial=False, proba_uniform=0, is_per_task=False):
        if is_per_task and (is_beta_binomial or proba_uniform):
            raise NotImplementedError("is_per_task draws uniform counts on the device; is_beta_binomial / proba_uniform "
                                      "are host-side draws of one size per batch")
        self.is_per_task = is_per_task
        self.last_counts = None
        self.a, self.b = a, b
        self.is_batch_share = is_batch_share
        self.range_indcs = range_indcs
        self.is_ensure_one = is_ensure_one
        self.is_beta_binomial = is_beta_binomial
        self.proba_uniform = proba_uniform

    def n_indcs(self, n_possible_points: int) -> int:
        if np.random.uniform(size=1) < self.proba_uniform:
            n = random.randint(0, n_possible_points)
        elif self.is_beta_binomial:
            from scipy.stats import betabinom

            n = int(betabinom(n_possible_points, self.a, self.b).rvs())
        else:
            n = random.randint(_point_count(self.a, n_possible_points), _point_count(self.b, n_possible_points))
        if self.is_ensure_one and n < 1:
            n = 1
        return n

    def __call__(self, batch_size, n_possible_points, device=None, generator: Optional[torch.Generator] = None, n_points=None):
        if n_points is not None and (not self.is_per_task or self.is_batch_share or self.range_indcs is not None):
            raise NotImplementedError("n_points (a padded data set) needs is_per_task=True and neither is_batch_share nor range_indcs")
        if self.range_indcs is not None:
            n_possible_points = self.range_indcs[1] - self.range_indcs[0]
        if self.is_per_task:
            lo, n = _point_count(self.a, n_possible_points), _point_count(self.b, n_possible_points)
            if self.is_ensure_one:
                lo, n = max(lo, 1), max(n, 1)
            self.last_counts = torch.randint(lo, n + 1, (batch_size,), device=device, generator=generator)
            if n_points is not None:
                n_points = n_points.to(device=self.last_counts.device, dtype=torch.int64).clamp(0, n_possible_points)
                self.last_counts = torch.minimum(self.last_counts, n_points)
        else:
            n = self.n_indcs(n_possible_points)
        if self.is_batch_share:
            indcs = torch.randperm(n_possible_points, device=device, generator=generator)[:n]
            indcs = indcs.unsqueeze(0).expand(batch_size, n)
        else:
            # an independent uniformly random subset (in random order) per row
            noise = torch.rand(batch_size, n_possible_points, device=device, generator=generator)
            if n_points is not None:  # (the padding points sort last: the first min(count, n_points) indices of a row are real points)
                beyond = torch.arange(n_possible_points, device=noise.device).unsqueeze(0) >= n_points.unsqueeze(1)
                noise = noise.masked_fill(beyond, float("inf"))
            indcs = noise.argsort(dim=1)[:, :n]
        if self.range_indcs is not None:
            indcs = indcs + self.range_indcs[0]
        return indcs


class CntxtTrgtGetter:
    """Split (X, y) into context and target points (datasplit.py:148-255): ``getter(X, y)`` ->
    ``X_cntxt, Y_cntxt, X_trgt, Y_trgt`` -- and, behind a ``contexts_getter`` with ``is_per_task=True``, a fifth value
    ``n_cntxt`` (int64 [B], on the device): the context comes padded to a fixed number of rows, task ``b`` owns the first
    ``n_cntxt[b]`` and the rows beyond are zero-filled; :meth:`batch` returns the same as the dict a model / ``Trainer.step`` takes.
    A ``targets_getter`` with ``is_per_task=True`` does the same for the targets: a sixth value ``n_trgt`` (the fifth is None when
    the contexts are not per-task), targets zero-filled beyond the count.  ``n_points=n`` (an integer device tensor [B]) splits a
    padded DATA SET, task ``b`` having ``n[b]`` real points out of ``X.shape[1]``: the per-task getters draw among those only,
    and with ``targets_getter=get_all_indcs`` the batch carries ``n_trgt = n``.  Nothing here reads a count on the host.
    Same constructor arguments, call signature and overridable hooks
    (``preprocess_context``, ``add_cntxts_to_trgts``, ``getter_inputs``, ``select``) as the reference; the work is
    two steps: :meth:`indices` decides which points go where (device-side draws unless the caller supplies them),
    :meth:`select` moves them (one gather launch per side)."""

    def __init__(self, contexts_getter=GetRandomIndcs(), targets_getter=get_all_indcs, is_add_cntxts_to_trgts=False):
        self.contexts_getter = contexts_getter
        self.targets_getter = targets_getter
        self.is_add_cntxts_to_trgts = is_add_cntxts_to_trgts

    def indices(self, X, context_indcs=None, target_indcs=None, n_points=None):
        """(context indices, target indices, were any supplied by the caller) for the batch ``X``."""
        batch_size, num_points = self.getter_inputs(X)
        supplied = not (context_indcs is None and target_indcs is None)
        drawn = []
        for given, getter in ((context_indcs, self.contexts_getter), (target_indcs, self.targets_getter)):
            if given is not None:
                drawn.append(given)
                continue
            if n_points is not None and getattr(getter, "is_per_task", False):
                drawn.append(getter(batch_size, num_points, device=X.device, n_points=n_points))
                continue
            try:
                drawn.append(getter(batch_size, num_points, device=X.device))
            except TypeError:  # a reference-style getter without the device argument
                drawn.append(getter(batch_size, num_points))
        ctx, trg = drawn
        if self.is_add_cntxts_to_trgts:
            trg = self.add_cntxts_to_trgts(num_points, trg, ctx)
        return ctx, trg, supplied

    def __call__(self, X, y=None, context_indcs=None, target_indcs=None, is_return_indcs=False, n_points=None):
        per_task_c = context_indcs is None and getattr(self.contexts_getter, "is_per_task", False)
        per_task_t = target_indcs is None and getattr(self.targets_getter, "is_per_task", False)
        all_t = target_indcs is None and self.targets_getter is get_all_indcs
        if self.is_add_cntxts_to_trgts and (per_task_t or n_points is not None):
            raise NotImplementedError("is_add_cntxts_to_trgts is not implemented with per-task targets or n_points")
        if n_points is not None:
            if not isinstance(n_points, torch.Tensor) or n_points.dtype not in (torch.int32, torch.int64) \
                    or tuple(n_points.shape) != (X.shape[0],):
                raise ValueError(f"n_points must be an integer tensor of shape [{X.shape[0]}] (the real points of every task)")
            if not (per_task_c and (per_task_t or all_t)):
                raise NotImplementedError("n_points needs a contexts getter with is_per_task=True and, as targets getter, "
                                          "get_all_indcs or a getter with is_per_task=True")
            n_points = n_points.to(device=X.device, dtype=torch.int64).clamp(0, X.shape[1])
        ctx, trg, supplied = self.indices(X, context_indcs, target_indcs, n_points=n_points)
        X_for_context = self.preprocess_context(X)
        if is_return_indcs:
            return ctx, X_for_context, trg, X
        # caller-supplied indices are range-checked (one host sync); the getters' own draws are in range by construction
        Xc, Yc = self.select(X_for_context, y, ctx, validate=supplied)
        Xt, Yt = self.select(X, y, trg, validate=supplied)
        n_cntxt = n_trgt = None
        if per_task_c:
            n_cntxt = self.contexts_getter.last_counts
            pad = (torch.arange(Xc.shape[1], device=Xc.device).unsqueeze(0) >= n_cntxt.unsqueeze(1)).unsqueeze(-1)
            Xc, Yc = Xc.masked_fill(pad, 0.0), Yc.masked_fill(pad, 0.0)
        if per_task_t or (n_points is not None and all_t):
            n_trgt = self.targets_getter.last_counts if per_task_t else n_points
            pad = (torch.arange(Xt.shape[1], device=Xt.device).unsqueeze(0) >= n_trgt.unsqueeze(1)).unsqueeze(-1)
            Xt, Yt = Xt.masked_fill(pad, 0.0), Yt.masked_fill(pad, 0.0)
        if n_trgt is not None:
            return Xc, Yc, Xt, Yt, n_cntxt, n_trgt
        if n_cntxt is not None:
            return Xc, Yc, Xt, Yt, n_cntxt
        return Xc, Yc, Xt, Yt

    def batch(self, X, y=None, **kwargs) -> dict:
        """The split as the dict ``Trainer.step`` / ``eval_loglike`` take: ``X_cntxt, Y_cntxt, X_trgt, Y_trgt`` and, with a
        per-task contexts getter, ``n_cntxt``; with a per-task targets getter or ``n_points`` (see the class), ``n_trgt``."""
        out = self(X, y, **kwargs)
        return {k: v for k, v in zip(("X_cntxt", "Y_cntxt", "X_trgt", "Y_trgt", "n_cntxt", "n_trgt"), out) if v is not None}

    # ---- hooks of the reference ---------------------------------------------------------------------------------
    def preprocess_context(self, X):
        """What the context side sees of X (identity; the reference's subclasses mask or crop here)."""
        return X

    def add_cntxts_to_trgts(self, num_points, target_indcs, context_indcs):
        """Targets followed by the context points, cut to ``num_points`` columns (datasplit.py:225-232)."""
        trg = torch.as_tensor(target_indcs)
        both = torch.cat([trg, torch.as_tensor(context_indcs).to(trg.device)], dim=-1)
        return both[:, :num_points]

    def getter_inputs(self, X):
        """(batch size, number of points) handed to the index getters."""
        return X.shape[0], X.shape[1]

    def select(self, X, y, indcs, validate=True):
        """``torch.gather`` of X and y along the points with the same indices (datasplit.py:246-255):
        one ``npf_gather_points`` launch.  ``validate``: range-check the indices (a host sync; the
        getters' own draws are in range by construction and skip it)."""
        if not X.is_cuda:
            raise RuntimeError("the HIP path takes device tensors only (got a CPU tensor); there is no CPU fallback")
        batch_size, num_points, x_dim = X.shape
        y_dim = y.size(-1)
        indcs = torch.as_tensor(indcs).to(device=X.device, dtype=torch.int64)
        if indcs.dim() != 2 or indcs.shape[0] != batch_size:
            raise ValueError(f"indices must be [batch_size, n_indcs], got {tuple(indcs.shape)}")
        indcs = indcs.contiguous()  # (materialises expanded / shared index rows)
        n_sel = indcs.shape[1]
        if validate and n_sel and (int(indcs.min()) < 0 or int(indcs.max()) >= num_points):
            raise IndexError("context / target index out of range")
        Xc, yc = X.contiguous().float(), y.contiguous().float()
        out_x = torch.empty(batch_size, n_sel, x_dim, dtype=torch.float32, device=X.device)
        out_y = torch.empty(batch_size, n_sel, y_dim, dtype=torch.float32, device=X.device)
        if n_sel:
            L.check(L.load().npf_gather_points(L.ptr(Xc), L.ptr(yc), indcs.data_ptr(), batch_size, num_points, n_sel,
                                               x_dim, y_dim, L.ptr(out_x), L.ptr(out_y), L.stream_ptr()),
                    "npf_gather_points")
        return out_x, out_y
