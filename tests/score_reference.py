"""float64 reference of the predictive scores (log density, PIT, CRPS of an equal-weight Gaussian mixture), the input regimes of
the score tests and the gates -- shared by tests/test_score_host.py (which checks this reference itself, on the CPU) and
tests/test_hip_score.py.  Not a test module.

Gates (per element): log density |d| <= 1e-5 max(1, |ref|); PIT |d| <= 1e-5; CRPS |d| <= 1e-5 |ref|."""
import math

import torch

GATE = 1e-5
REGIMES = ("random", "spread_tiny_sigma", "offset_close", "far_y", "mixed_sigma", "identical")
RAW_TINY = -40.0                      # raw scale whose sigma is 0.01 (softplus(-40) = 4e-18)
RAW_30 = (30.0 - 0.01) / 0.99         # raw scale whose sigma is 30 (softplus(x) = x there)


def sigma_of(raw):
    """The head's scale, 0.01 + 0.99 softplus(raw), in the dtype of ``raw``."""
    return 0.01 + 0.99 * torch.where(raw > 30.0, raw, torch.log1p(torch.exp(raw.clamp(max=30.0))))


def _A(m, s):
    return 2.0 * s * torch.exp(-0.5 * (m / s) ** 2) / math.sqrt(2.0 * math.pi) + m * torch.erf(m / (s * math.sqrt(2.0)))


def scores(mu, sg, y):
    """(log_density, pit, crps) of the mixture of N(mu[k], sg[k]^2), k over axis 0, at ``y`` (the shape of mu[0]); the closed forms of
    the issue evaluated in the dtype of the arguments (float64: the reference; float32: the plain evaluation of the host test)."""
    K = mu.shape[0]
    u = (y.unsqueeze(0) - mu) / sg
    ld = torch.logsumexp(-0.5 * u * u - sg.log() - 0.5 * math.log(2.0 * math.pi), 0) - math.log(K)
    pit = (0.5 * torch.special.erfc(-u / math.sqrt(2.0))).mean(0)
    pair = _A(mu.unsqueeze(0) - mu.unsqueeze(1), (sg.unsqueeze(0) ** 2 + sg.unsqueeze(1) ** 2).sqrt())
    crps = _A(y.unsqueeze(0) - mu, sg).mean(0) - 0.5 * pair.mean((0, 1))
    return ld, pit, crps


def regime(name, n_z, n, seed):
    """(mu, raw, y) float32 CPU tensors [n_z, n], [n_z, n], [n]: ``n`` elements of the named regime (the head makes sigma of raw)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if name == "random":
        mu, raw, y = rn(n_z, n), rn(n_z, n), 1.5 * rn(n)
    elif name == "spread_tiny_sigma":  # y at a component
        mu, raw = 100.0 * rn(n_z, n), torch.full((n_z, n), RAW_TINY)
        y = mu[torch.arange(n) % n_z, torch.arange(n)].clone()
    elif name == "offset_close":
        mu, raw = 1e3 + 1e-3 * torch.sign(rn(n_z, n)), torch.full((n_z, n), RAW_TINY)
        y = 1e3 + 5e-3 * rn(n)
    elif name == "far_y":
        mu, raw = rn(n_z, n), rn(n_z, n)
        y = 50.0 * torch.sign(rn(n)) + rn(n)
    elif name == "mixed_sigma":
        mu, raw, y = 3.0 * rn(n_z, n), torch.where(torch.rand(n_z, n, generator=g) < 0.5, RAW_TINY, RAW_30), 3.0 * rn(n)
    elif name == "identical":
        mu, raw = rn(1, n).expand(n_z, n).contiguous(), rn(1, n).expand(n_z, n).contiguous()
        y = mu[0].clone()
    else:
        raise KeyError(name)
    return mu.float(), raw.float(), y.float()


def ratios(got, ref, live=None):
    """Worst error / gate per quantity over the elements ``live`` selects: ``got`` / ``ref`` are (log_density, pit, crps), an entry of
    ``got`` may be None.  -> dict name -> ratio (<= 1 passes)."""
    out = {}
    for name, g, r in zip(("log_density", "pit", "crps"), got, ref):
        if g is None:
            continue
        g, r = g.double().reshape(-1), r.double().reshape(-1).to(g.device)
        if live is not None:
            g, r = g[live.reshape(-1)], r[live.reshape(-1)]
        if g.numel() == 0:
            out[name] = 0.0
            continue
        gate = {"log_density": GATE * r.abs().clamp(min=1.0), "pit": torch.full_like(r, GATE), "crps": GATE * r.abs()}[name]
        d = (g - r).abs()
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))  # (a NaN never passes)
        out[name] = float((d / gate).max())
    return out
