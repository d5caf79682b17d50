"""Helpers shared by the tests: build this package's models for a golden case."""
import contextlib
import warnings
from functools import partial

import numpy as np
import torch
from torch.distributions import Independent, Normal

import specs


class EpsIndependent(Independent):
    """Independent(Normal) whose rsample uses an injected eps (the same device-side
    replacement of the global-RNG draw that make_golden.py applies to the reference)."""

    eps = None

    def rsample(self, sample_shape=torch.Size()):
        e = type(self).eps
        assert e is not None and e.shape[0] == sample_shape[0]
        return self.base_dist.loc + e * self.base_dist.scale


def eps_latent_dist(loc, scale):
    return EpsIndependent(Normal(loc, scale, validate_args=False), 1)


def build_model(case: dict, device="cuda:0", params=None):
    import npf_gwwaveform_amd as A

    r = case["r"]
    res, drop = case.get("is_res", False), case.get("dropout", 0)
    kw = dict(
        r_dim=r, is_heteroskedastic=case.get("is_heteroskedastic", True),
        XYEncoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=case["L_xy"], is_force_hid_smaller=True,
                                             hidden_size=r, is_res=res, dropout=drop),
                                     is_sum_merge=case.get("is_sum_merge", True)),
        Decoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=case["L_dec"], hidden_size=r, is_res=res, dropout=drop),
                                   is_sum_merge=True),
    )
    if "x_transf_dim" in case:
        kw["x_transf_dim"] = case["x_transf_dim"]
    kind = case["kind"]
    if kind in ("LNP", "AttnLNP"):
        n_z = case.get("n_z", 1)
        kw.update(is_q_zCct=case.get("is_q_zCct", False), n_z_samples_train=n_z, n_z_samples_test=n_z,
                  LatentDistribution=eps_latent_dist)
    if kind == "LNP":
        kw["encoded_path"] = case["encoded_path"]
    if "attention" in case:
        kw["attention"] = case["attention"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = getattr(A, kind)(case["dx"], case["dy"], **kw)
    m.load_state_dict(params if params is not None else specs.make_params(case), strict=True)
    return m.to(device)


def build_loss(case: dict):
    import npf_gwwaveform_amd as A

    return {"cnpf": A.CNPFLoss, "elbo": A.ELBOLossLNPF, "nll": A.NLLLossLNPF,
            "sumo": A.SUMOLossLNPF}[specs.loss_name(case)]()


def assert_close(got, ref, tol=1e-5, what=""):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    m = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max()
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    assert err <= tol * m, f"{what}: max|d|={err:.3e} > {tol:.0e} * max|ref|={m:.3e}"


class _RecordingLib:
    """Stands in for the loaded ``libnpf_hip.so`` handle: every ``npf_*`` attribute fetched through it is wrapped so that a call
    counts under its name before it runs.  Everything else passes through."""

    def __init__(self, lib, counts):
        self._real, self._counts = lib, counts

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("npf_"):
            return fn
        counts = self._counts

        def call(*args):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args)

        return call


class LaunchWitness:
    """What a block of code launched: ``calls`` maps each C-ABI entry point (``npf_chain_run``, ``npf_x6_run_ex``, ...) to the
    number of times it was called, ``spied`` each spied Python function (``"module.attr"``) likewise."""

    def __init__(self):
        self.calls, self.spied = {}, {}

    def __getitem__(self, name):
        return self.calls.get(name, 0) if name.startswith("npf_") else self.spied.get(name, 0)

    def reset(self):
        self.calls.clear()
        self.spied.clear()

    def __repr__(self):
        return f"LaunchWitness({dict(sorted(self.calls.items()))}, spied={dict(sorted(self.spied.items()))})"


@contextlib.contextmanager
def launch_witness(spy=()):
    """Record every entry point of the HIP library called inside the block.  Every launch of the package goes through
    ``_lib.load().npf_xxx(...)`` at call time, so swapping the cached handle for a recording proxy sees all of them; the real
    handle is put back on exit, also when the block raises.  ``spy``: names ``"module.attr"`` of functions of the package
    (looked up at call time by their callers) whose calls are counted too, e.g. ``"attention_long.long_scaledot_attention"``."""
    import importlib

    from npf_gwwaveform_amd import _lib as L

    w = LaunchWitness()
    real = L.load()
    patched = []
    try:
        for name in spy:
            mod_name, attr = name.rsplit(".", 1)
            mod = importlib.import_module(f"npf_gwwaveform_amd.{mod_name}")
            orig = getattr(mod, attr)

            def counted(*a, _orig=orig, _name=name, **kw):
                w.spied[_name] = w.spied.get(_name, 0) + 1
                return _orig(*a, **kw)

            patched.append((mod, attr, orig))
            setattr(mod, attr, counted)
        L._lib = _RecordingLib(real, w.calls)
        yield w
    finally:
        L._lib = real
        for mod, attr, orig in reversed(patched):
            setattr(mod, attr, orig)
