"""Host side of the differentiable matched-filter likelihood (CPU, no kernel launched): the float64 closed form of
tests/loglike_grad_reference.py against central differences of the definition in 50-digit arithmetic, the kernels' order of
operations (``recurrence``) against the gate on every input set of the GPU suite, the I1 / I0 scheme against 50 digits, the runner-up
margin that makes the ``lnl_max`` gradient well posed, the refusals of the Python layer and the new symbols of the C ABI."""
import ctypes as C
import math
import os
import re

import mpmath
import pytest
import torch

import loglike_grad_reference as G
import loglike_net_reference as RN
import loglike_reference as R1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JC, X_S = 16, 24.0
mpmath.mp.dps = 50


# ---- the closed form against the definition in 50 digits ----------------------------------------------------------------------------
def _mp_rows(args):
    """Per row r: a function ``h_row [T][2] (mpf) -> (lnl_marg, lnl_max)`` of the definition in mpmath, over the live points."""
    mp = mpmath.mp
    net = "response" in args
    h = args["h"]
    Rn, T = h.shape[:2]
    data = args["data"].double() if net else args["data"].double().unsqueeze(1)
    Bn, D = data.shape[:2]
    w = args["weights"]
    if w is None:
        w = torch.ones(Bn, D, T, dtype=torch.float64)
    elif net:
        w = w.double().expand(Bn, D, T)
    else:
        w = w.double().expand(Bn, T).unsqueeze(1)
    f = torch.zeros(Bn, T, dtype=torch.float64) if args["freqs"] is None else args["freqs"].double().expand(Bn, T)
    resp = args["response"] if net else torch.tensor([1.0, 0.0], dtype=torch.float64).expand(Bn, 1, 2)
    dl = args["delays"] if net and args["delays"] is not None else torch.zeros(Bn, D, dtype=torch.float64)
    nv = [T] * Bn if args["n_valid"] is None else [min(max(int(v), 0), T) for v in args["n_valid"]]
    taus = args["taus"]
    grid = [mp.mpf(0)] if taus is None else [mp.mpf(taus[0]) + j * mp.mpf(taus[1]) for j in range(taus[2])]
    two_pi = 2 * mp.pi

    def make(r):
        b = r % Bn

        def lnl(row):
            Ks = [mp.mpc(0)] * len(grid)
            HH = mp.mpf(0)
            for k in range(D):
                Ck = mp.mpc(float(resp[b, k, 0]), float(resp[b, k, 1]))
                for t in range(nv[b]):
                    wt = float(w[b, k, t])
                    if not (wt > 0 and math.isfinite(wt)):
                        continue
                    A, ph = row[t]
                    c = mp.mpf(wt) * A * mp.mpc(float(data[b, k, t, 0]), -float(data[b, k, t, 1]))
                    HH += abs(Ck) ** 2 * mp.mpf(wt) * A * A
                    for j, tau in enumerate(grid):
                        Ks[j] = Ks[j] + Ck * c * mp.expjpi(2 * (ph / two_pi + mp.mpf(float(f[b, t])) * (tau + mp.mpf(float(dl[b, k])))))
            xs = [abs(K) for K in Ks]
            marg = mp.log(mp.fsum(mp.besseli(0, x) for x in xs) / len(grid)) - HH / 2
            return marg, max(xs) - HH / 2

        return lnl

    return [make(r) for r in range(Rn)], Bn


def _mp_gradient(args, ups, step="1e-18"):
    """d F / d h [R, T, 2] by central differences in mpmath, F = sum_r (d_marg lnl_marg + d_max lnl_max) + sum_b (d_mix lnl_mix +
    d_max_mix lnl_max_mix)."""
    mp = mpmath.mp
    rows, Bn = _mp_rows(args)
    h = args["h"]
    Rn, T = h.shape[:2]
    n_z = Rn // Bn
    hm = [[(mp.mpf(float(h[r, t, 0])), mp.mpf(float(h[r, t, 1]))) if math.isfinite(float(h[r, t, 0])) else (mp.mpf(0), mp.mpf(0))
           for t in range(T)] for r in range(Rn)]
    base = [rows[r](hm[r]) for r in range(Rn)]
    get = lambda k, i: mp.mpf(float(ups[k][i])) if ups.get(k) is not None else mp.mpf(0)  # noqa: E731

    def F_of_task(b, vals):
        lme = lambda v: mp.log(mp.fsum(mp.exp(x) for x in v) / n_z)  # noqa: E731
        out = get("d_mix", b) * lme([vals[s * Bn + b][0] for s in range(n_z)]) + \
            get("d_max_mix", b) * lme([vals[s * Bn + b][1] for s in range(n_z)])
        for s in range(n_z):
            r = s * Bn + b
            out += get("d_marg", r) * vals[r][0] + get("d_max", r) * vals[r][1]
        return out

    eps = mp.mpf(step)
    grad = torch.zeros(Rn, T, 2, dtype=torch.float64)
    for r in range(Rn):
        for t in range(T):
            for e in range(2):
                val = []
                for sign in (1, -1):
                    row = list(hm[r])
                    pt = list(row[t])
                    pt[e] += sign * eps
                    row[t] = tuple(pt)
                    vals = list(base)
                    vals[r] = rows[r](row)
                    val.append(F_of_task(r % Bn, vals))
                grad[r, t, e] = float((val[0] - val[1]) / (2 * eps))
    return grad


def _fd_cases():
    out = []
    for n_tau in (None, 1, 3):
        taus = None if n_tau is None else (-R1.DTAU, R1.DTAU, n_tau)
        case = R1.build("noise", 5, n_z=2, h_ld=2, wform="BT", fform="T", taus=taus, counts=(5, 4, 5), seed=3)
        out.append((f"single n_tau={n_tau}", R1.call_args(case)))
    case = RN.build("noise", 5, D=2, n_z=2, h_ld=4, wform="BT", fform="BT", taus=(-R1.DTAU, R1.DTAU, 3), seed=4)
    assert case["delays"] is not None
    out.append(("network D=2 n_tau=3 with delays", RN.call_args(case)))
    case = RN.build("noise", 5, D=2, n_z=2, h_ld=2, wform="T", fform="T", taus=None, seed=5)
    out.append(("network D=2 no grid with delays", RN.call_args(case)))
    return out


@pytest.mark.parametrize("kind", ("marg", "mix", "all"))
def test_closed_form_equals_central_differences_of_the_definition_in_50_digits(kind):
    """T = 5, n_tau in {none, 1, 3}, n_z = 2, and a network of two detectors with delays: |closed form - finite difference| <=
    1e-12 S_{r,t}.  The ``lnl_max`` gradient enters with ``all``; the cases leave its maximiser clear."""
    for i, (tag, args) in enumerate(_fd_cases()):
        parts = G.closed_form(args)
        Rn = args["h"].shape[0]
        ups = G.upstream(kind, Rn, parts.Bn, i)
        if kind == "all":
            assert G.clear_maximum(parts.ref), tag
        want, S = G.grad_of(parts, ups)
        fd = _mp_gradient(args, ups)
        bound = 1e-12 * S.unsqueeze(-1)
        d = (want - fd).abs()
        worst = float(torch.where(d == 0, torch.zeros_like(d), d / bound).max())
        print(f"LNLGRAD closed form against 50-digit differences, {tag}, upstream {kind}: worst / (1e-12 S) {worst:.3g}")
        assert float(want.abs().max()) > 0 and worst <= 1.0, (tag, kind, worst)


# ---- the kernels' order of operations against the gate ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def suite():
    """(tag, args, closed form, recurrence) of every input set of the GPU suite."""
    out = []
    for tag, fac, args in G.cases(JC, X_S) + [("net " + t, f, a) for t, f, a in G.net_cases(JC, X_S)]:
        out.append((tag, args, G.closed_form(args), G.recurrence(args, JC, X_S)))
    return out


def test_recurrence_stays_below_a_tenth_of_the_gate_on_every_case_of_the_gpu_suite(suite):
    worst, where = 0.0, None
    for i, (tag, args, closed, rec) in enumerate(suite):
        Rn = args["h"].shape[0]
        for kind in G.UPSTREAMS:
            ups = G.upstream(kind, Rn, closed.Bn, i)
            want, S = G.grad_of(closed, ups)
            got, _ = G.grad_of(rec, ups)
            gate = ((1e-10 * R1.scale_of(closed.ref) + 1e-12).view(-1, 1) * S).unsqueeze(-1)  # (no fp32 rounding on the CPU)
            d = (got - want).abs()
            r = float(torch.where(d == 0, torch.zeros_like(d), d / gate).max())
            if r > worst:
                worst, where = r, f"{tag} upstream {kind}"
    print(f"LNLGRAD recurrence against the closed form over {len(suite)} cases: worst error / gate {worst:.3g} ({where})")
    assert len(suite) >= 100 and worst <= 0.1, (worst, where)


def test_every_case_leaves_the_maximiser_clear(suite):
    """The runner-up of max_j x_j lies at least 1e3 forward gates below the best in every case: the ``lnl_max`` gradient, taken at
    the index the forward finds, is well posed, and the closed form and the recurrence agree on the index."""
    for tag, args, closed, rec in suite:
        assert G.clear_maximum(closed.ref), tag
        assert torch.equal(closed.ref["tau_index"], rec.ref["tau_index"]), tag


# ---- I1 / I0 ------------------------------------------------------------------------------------------------------------------------
def test_rho_scheme_meets_50_digits_to_2e_15_on_both_sides_of_the_switch():
    mp = mpmath.mp
    xs = [1e-300, 1e-8, 1e-3, 0.5, 1.0, 3.0, 10.0, 20.0, 23.5, 23.999, math.nextafter(X_S, 0.0), X_S, math.nextafter(X_S, 100.0), 24.001,
          25.0, 30.0, 100.0, 1e3, 1e6, 1e12]
    xs += [10.0 ** (-6 + 0.37 * i) for i in range(40)]
    worst = 0.0
    for x in xs:
        want = mp.besseli(1, mp.mpf(x)) / mp.besseli(0, mp.mpf(x))
        got = G.rho_scheme(x, X_S)
        worst = max(worst, float(abs(mp.mpf(got) - want) / want))
        assert 0.0 < got < 1.0 or x >= 1e6, x
    print(f"LNLGRAD I1 / I0 scheme against 50 digits: worst relative error {worst:.3g}")
    assert worst <= 2e-15
    assert G.rho_scheme(0.0, X_S) == 0.0 and G.rho_scheme(1e300, X_S) == 1.0 and math.isfinite(G.rho_scheme(1e-320, X_S))


def test_rho_is_the_derivative_of_the_kernels_log_i0():
    """Central difference of ``log_i0_scheme`` with step 1e-4 max(x, 1): the rounding of the difference costs 2^-52 ln I0 / step <=
    3e-12, the truncation step^2 |rho''| / 6 <= 2e-9: the bound is 1e-8 absolute (rho <= 1)."""
    for x in (1e-2, 0.3, 1.0, 5.0, 23.0, 23.9999, 24.0001, 30.0, 500.0):
        step = 1e-4 * max(x, 1.0)
        fd = (R1.log_i0_scheme(x + step, X_S) - R1.log_i0_scheme(x - step, X_S)) / (2 * step)
        assert abs(fd - G.rho_scheme(x, X_S)) <= 1e-8, x


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_functional_calls_refuse_what_the_contract_lists():
    from npf_gwwaveform_amd import functional as FN

    h, d, w, f = torch.zeros(6, 5, 4), torch.zeros(3, 5, 2), torch.ones(5), torch.ones(5)
    taus = (0.0, 1e-3, 3)
    for name in ("data", "weights", "freqs"):
        kw = dict(data=d, weights=w, freqs=f)
        kw[name] = kw[name].clone().requires_grad_()
        with pytest.raises(ValueError, match=f"no gradient with respect to {name}"):
            FN.waveform_lnl(h, taus=taus, **kw)
    with pytest.raises(ValueError, match="n_bcast"):
        FN.waveform_lnl(h, d, w, f, taus, n_bcast=2)
    with pytest.raises(ValueError, match="n_bcast"):
        FN.waveform_lnl(h, d, n_bcast=0)
    with pytest.raises(ValueError, match="mean must have shape"):
        FN.waveform_lnl(h, d, n_bcast=2, mean=torch.zeros(6, 5, 2))
    with pytest.raises(ValueError, match="needs freqs"):
        FN.waveform_lnl(h, d, taus=taus)
    with pytest.raises(RuntimeError, match="fp32 device tensors"):
        FN.waveform_lnl(h, d, w, f, taus)  # (CPU tensors)
    with pytest.raises(RuntimeError, match="fp32 device tensors"):
        FN.waveform_lnl(h.double(), d)
    dn, resp, dl, wn = torch.zeros(3, 2, 5, 2), torch.zeros(3, 2, 2, dtype=torch.float64), torch.zeros(3, 2, dtype=torch.float64), torch.ones(2, 5)
    for name in ("data", "response", "delays", "weights", "freqs"):
        kw = dict(data=dn, response=resp, delays=dl, weights=wn, freqs=f)
        kw[name] = kw[name].clone().requires_grad_()
        with pytest.raises(ValueError, match=f"no gradient with respect to {name}"):
            FN.waveform_lnl_network(h, taus=taus, **kw)
    with pytest.raises(ValueError, match="n_bcast"):
        FN.waveform_lnl_network(h, dn, resp, n_bcast=3)
    with pytest.raises(ValueError, match="float64"):
        FN.waveform_lnl_network(h, dn, resp.float())
    with pytest.raises(ValueError, match="delays need freqs"):
        FN.waveform_lnl_network(h, dn, resp, dl)
    with pytest.raises(RuntimeError, match="fp32 device tensors"):
        FN.waveform_lnl_network(h, dn, resp, dl, wn, f, taus)


def test_head_distribution_and_loss_argument_checks():
    import npf_gwwaveform_amd as A

    p = A.HeadDistribution(torch.zeros(3, 5, 2), 1, False, 1, 3, 5)
    with pytest.raises(ValueError, match="y_dim"):
        p.lnl(torch.zeros(3, 5, 2))
    with pytest.raises(ValueError, match="y_dim"):
        p.lnl_network(torch.zeros(3, 2, 5, 2), torch.zeros(3, 2, 2, dtype=torch.float64))
    p2 = A.HeadDistribution(torch.zeros(3, 5, 4), 2, False, 1, 3, 5)
    with pytest.raises(ValueError, match="of must be"):
        p2.lnl(torch.zeros(3, 5, 2), of="median")
    with pytest.raises(ValueError, match="data"):
        p2.lnl(torch.zeros(3, 4, 2))
    f = torch.ones(5)
    for bad in (dict(base=3), dict(lam=float("nan")), dict(lam=torch.tensor(1.0)), dict(statistic="mean"), dict(of="median"),
                dict(reduction="max"), dict(weights=torch.ones(5, dtype=torch.float64)), dict(freqs=torch.ones(1, 1, 5)),
                dict(freqs=torch.ones(5, requires_grad=True)), dict(taus=(0.0, 1e-3, 3)), dict(freqs=f, taus=(0.0, 1e-3, 0)),
                dict(noise=torch.zeros(3, 5)), dict(noise=torch.zeros(3, 5, 2, dtype=torch.float64)),
                dict(noise=torch.zeros(3, 5, 2, requires_grad=True))):
        with pytest.raises(ValueError):
            A.LogLikeLoss(**bad)
    crit = A.LogLikeLoss(base=A.CNPFLoss(), lam=2, weights=torch.ones(5), freqs=f, taus=(0.0, 1e-3, 3), statistic="max", of="mean",
                         noise=torch.zeros(3, 5, 2))
    assert crit.lam == 2.0 and crit.taus == (0.0, 1e-3, 3) and not crit.state_dict()  # (the buffers are not persistent)
    assert {k for k, _ in crit.named_buffers()} == {"weights", "freqs", "noise"}
    with pytest.raises(ValueError, match="predictive distribution"):
        crit((torch.distributions.Normal(0.0, 1.0), None, None, None), torch.zeros(3, 5, 2))
    # the injection: A' e^{i phi'} with the sines in double, rounded once, plus the noise
    Y = torch.tensor([[[2.0, 1e4 + 0.25], [0.5, -3.0]]])
    crit = A.LogLikeLoss(noise=torch.tensor([[[0.5, -1.0], [0.0, 0.0]]]))
    want = torch.tensor([[[2.0 * math.cos(1e4 + 0.25) + 0.5, 2.0 * math.sin(1e4 + 0.25) - 1.0], [0.5 * math.cos(-3.0), 0.5 * math.sin(-3.0)]]],
                        dtype=torch.float64).float()
    assert torch.equal(crit.injection(Y), want) and not crit.injection(Y.requires_grad_()).requires_grad


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
HEAD = ["h", "h_ld", "d", "wgt", "wgt_rows", "freq", "freq_rows", "n_valid"]
SIZES = ["n_rows", "n_tasks", "pts", "tau0", "dtau", "n_tau"]
NET_SIZES = ["delay", "resp", "n_rows", "n_tasks", "n_det", "pts", "tau0", "dtau", "n_tau"]
OUTS = ["hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "series", "lnl_mix", "lnl_max_mix"]
BWD = ["tau_index", "saved", "lnl_marg", "lnl_max", "lnl_mix", "lnl_max_mix", "d_marg", "d_max", "d_mix", "d_max_mix", "n_bcast", "d_h",
       "dh_ld", "stream"]


def _declared(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/npf_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_new_entry_points_are_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    names = {"npf_waveform_loglike_ex": HEAD + SIZES + OUTS + ["saved", "workspace", "stream"],
             "npf_waveform_loglike_net_ex": HEAD + NET_SIZES + OUTS + ["hh_det", "snr_det", "dd_det", "saved", "workspace", "stream"],
             "npf_waveform_loglike_bwd": HEAD + SIZES + BWD,
             "npf_waveform_loglike_net_bwd": HEAD + NET_SIZES + BWD}
    for name, want in names.items():
        decl = _declared(header, name)
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl) == len(want) and hasattr(lib, name), name
        assert [a.split()[-1].lstrip("*") for a in decl] == want, name
        for a, t in zip(decl, args):
            assert t is (C.c_void_p if "*" in a else C.c_double if a.startswith("double") else C.c_int32), (name, a, t)
    for parent in ("npf_waveform_loglike", "npf_waveform_loglike_net"):  # the parent's argument list plus ``saved`` before workspace
        ex = _declared(header, parent + "_ex")
        assert _declared(header, parent) == ex[:-3] + ex[-2:] and ex[-3] == "double *saved", parent
    assert re.search(r"\bint64_t\s+npf_waveform_loglike_saved_doubles\s*\(int32_t n_tau\)\s*;", header)
    assert L.SIGNATURES["npf_waveform_loglike_saved_doubles"] == (C.c_int64, [C.c_int32])
    fn = lib.npf_waveform_loglike_saved_doubles
    fn.restype, fn.argtypes = C.c_int64, [C.c_int32]
    assert [fn(n) for n in (0, 1, 17, 65536, 65537, -1)] == [6, 6, 38, 4 + 2 * 65536, -1, -1]
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)
