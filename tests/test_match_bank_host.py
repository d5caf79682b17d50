"""Host side of the bank match (CPU, no kernel launched): the C ABI of ``npf_waveform_match_bank`` and its refusals, the refusals of
``functional.waveform_match_bank`` / ``HeadDistribution.match_bank``, and the float64 reference of tests/match_bank_reference.py
itself -- its columns against ``match_reference.reference`` on one template broadcast over the tasks, and the runner-up margins (over
the shifts of every pair, over the templates of every row) of every input set the GPU test uses."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import match_bank_reference as RB
import match_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["h", "h_ld", "bank", "wgt", "freq", "n_rows", "n_bank", "pts", "tau0", "dtau", "n_tau", "hh", "gg", "match", "mismatch",
         "tau_index", "phase", "dot", "best_index", "best_match", "workspace", "stream"]


@pytest.fixture(scope="module")
def all_cases():
    return [(tag, fac, case, RB.reference(**RB.call_args(case))) for tag, fac, case in RB.cases()]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_match_bank_is_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    m = re.search(r"\bint\s+npf_waveform_match_bank\s*\(([^;]*)\)\s*;", header)
    assert m, "npf_waveform_match_bank is not declared in include/npf_hip.h"
    decl = [a.strip() for a in m.group(1).split(",")]
    res, args = L.SIGNATURES["npf_waveform_match_bank"]
    assert res is C.c_int and len(args) == len(decl) == len(NAMES) and hasattr(lib, "npf_waveform_match_bank")
    for a, t in zip(decl, args):
        assert t is (C.c_void_p if "*" in a else C.c_double if a.startswith("double") else C.c_int32), (a, t)
    assert [a.split()[-1].lstrip("*") for a in decl] == NAMES
    assert "double *dot" in m.group(1) and "int32_t *best_index" in m.group(1) and "int32_t *tau_index" in m.group(1)
    assert re.search(r"\bint64_t\s+npf_waveform_match_bank_workspace_bytes\s*\(\s*int32_t n_rows,\s*int32_t n_bank,\s*int32_t pts,"
                     r"\s*int32_t n_tau\s*\)\s*;", header)
    assert L.SIGNATURES["npf_waveform_match_bank_workspace_bytes"] == (C.c_int64, [C.c_int32] * 4)
    assert hasattr(lib, "npf_waveform_match_bank_workspace_bytes")
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)


def test_workspace_bytes_and_refusals_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    ws = lib.npf_waveform_match_bank_workspace_bytes
    small, big = ws(3, 5, 37, 5), ws(33, 40, 129, 17)
    assert 0 < small < big
    # at least the two operand panels in double and the rotations of every chunk
    assert big >= 16 * 129 * (33 + 40) + 16 * 129 * 3
    assert ws(1 << 24, 1 << 20, 4, 0) > 0  # (the largest sizes: no overflow of the byte count)
    for bad in ((0, 5, 37, 5), (3, 0, 37, 5), (3, 5, 0, 5), (-1, 5, 37, 5), (3, -1, 37, 5), (3, 5, -1, 5), ((1 << 24) + 1, 5, 37, 5),
                (3, (1 << 20) + 1, 37, 5), (3, 5, 37, -1), (3, 5, 37, 65537)):
        assert ws(*bad) == -1, bad
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    ok = dict(h=p, h_ld=2, bank=p, wgt=p, freq=p, n_rows=6, n_bank=2, pts=4, tau0=0.0, dtau=1e-3, n_tau=3, hh=p, gg=p, match=p, mismatch=p,
              tau_index=p, phase=p, dot=p, best_index=p, best_match=p, workspace=p)
    assert list(ok) == NAMES[:-1]
    none = dict(hh=None, gg=None, match=None, mismatch=None, tau_index=None, phase=None, dot=None, best_index=None, best_match=None)
    for change in (dict(n_rows=0), dict(n_rows=-3), dict(n_bank=0), dict(pts=0), dict(n_rows=(1 << 24) + 1), dict(n_bank=(1 << 20) + 1),
                   dict(h_ld=1), dict(h_ld=0), dict(n_tau=-1), dict(n_tau=65537), dict(freq=None), none, dict(workspace=None), dict(h=None),
                   dict(bank=None)):
        a = dict(ok, **change)
        assert lib.npf_waveform_match_bank(*a.values(), None) == -1, change


def test_signatures_and_exports():
    import npf_gwwaveform_amd as A

    FN = A.functional
    assert list(inspect.signature(FN.waveform_match_bank).parameters) == ["h", "bank", "weights", "freqs", "taus", "want", "dot"]
    assert inspect.signature(FN.waveform_match_bank).parameters["want"].default == FN.BANK_NAMES
    assert FN.WaveformBankMatch._fields == FN.BANK_NAMES + ("dot",)
    assert list(inspect.signature(A.HeadDistribution.match_bank).parameters)[1:] == ["bank", "weights", "freqs", "taus", "of", "dot"]
    assert inspect.signature(A.HeadDistribution.match_bank).parameters["of"].default == "samples"
    assert A.BankMatch._fields == ("match", "mismatch", "tau", "tau_index", "phase", "best_index", "best_match", "dot")
    assert "BankMatch" in A.__all__ and "BankMatch" in A.neuralproc.__all__ and A.BankMatch is A.neuralproc.BankMatch


def test_every_listed_value_error_names_its_argument_and_comes_before_the_device_check():
    import npf_gwwaveform_amd as A

    FN = A.functional
    T, G = 5, 3
    h, bank, w, f = torch.zeros(4, T, 2), torch.zeros(G, T, 2), torch.ones(T), torch.ones(T)
    p = A.HeadDistribution(torch.zeros(4, T, 4), 2, False, 2, 2, T)
    bad = [
        (dict(bank=torch.zeros(G, T, 3)), "bank"), (dict(bank=torch.zeros(G, T + 1, 2)), "bank"), (dict(bank=torch.zeros(T, 2)), "bank"),
        (dict(bank=torch.zeros(0, T, 2)), "bank"), (dict(bank=[1.0]), "bank"),
        (dict(weights=torch.ones(T + 1)), "weights"), (dict(weights=torch.ones(G, T)), "weights"), (dict(weights=torch.ones(4, T)), "weights"),
        (dict(freqs=torch.ones(T - 1), taus=(0.0, 1e-3, 4)), "freqs"), (dict(freqs=torch.ones(G, T)), "freqs"),
        (dict(taus=(0.0, 1e-3, 4)), "freqs"),  # taus without freqs
        (dict(freqs=f, taus=(0.0, 1e-3, 0)), "taus"), (dict(freqs=f, taus=(0.0, 1e-3, 65537)), "taus"),
        (dict(freqs=f, taus=(math.inf, 1e-3, 4)), "taus"), (dict(freqs=f, taus=(0.0, 1e-3)), "taus"),
        (dict(freqs=f, taus=torch.tensor([0.0, 1e-3, 4.0])), "taus"),
    ]
    for kw, name in bad:
        with pytest.raises(ValueError, match=name):
            FN.waveform_match_bank(h, **dict(dict(bank=bank), **kw))
        with pytest.raises(ValueError, match=name):
            p.match_bank(**dict(dict(bank=bank), **kw))
        with pytest.raises(ValueError, match=name):
            FN.check_match_bank_args(h.shape, **dict(dict(bank=bank), **kw))
    for hb in (torch.zeros(4, T, 1), torch.zeros(4, T), torch.zeros(0, T, 2)):
        with pytest.raises(ValueError, match="h must"):
            FN.waveform_match_bank(hb, bank)
    with pytest.raises(ValueError, match="rows"):
        FN.check_match_bank_args(((1 << 24) + 1, T, 2), bank)
    for want in (("matches",), "match", None, ()):
        with pytest.raises(ValueError, match="want"):
            FN.waveform_match_bank(h, bank, want=want)
    assert FN.check_match_bank_args(h.shape, bank, w, f, (0.5, 1e-3, 4)) == (4, T, 2, G, 0.5, 1e-3, 4)
    assert FN.check_match_bank_args(h.shape, bank) == (4, T, 2, G, 0.0, 0.0, 0)
    with pytest.raises(ValueError, match="y_dim"):
        A.HeadDistribution(torch.zeros(4, T, 2), 1, False, 2, 2, T).match_bank(bank)
    with pytest.raises(ValueError, match="of must be"):
        p.match_bank(bank, of="median")
    padded = A.HeadDistribution(torch.zeros(4, T, 4), 2, False, 2, 2, T, n_trgt=torch.tensor([T, 2], dtype=torch.int32))
    for of in ("samples", "mean"):
        with pytest.raises(ValueError, match="one shared grid"):
            padded.match_bank(bank, of=of)
    # and once everything fits, the device check: there is no CPU path
    for kw in (dict(), dict(weights=w, freqs=f, taus=(0.0, 1e-3, 4)), dict(dot=True, want=())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FN.waveform_match_bank(h, bank, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.match_bank(bank, weights=w)
    assert p._base is None


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_cases_sit_on_every_boundary_the_issue_lists(all_cases):
    seen = {k: {fac[k] for _, fac, _, _ in all_cases} for k in ("n_rows", "n_bank", "pts", "n_tau", "h_ld", "weighted")}
    assert set(RB.ROWS) <= seen["n_rows"] and set(RB.BANKS) <= seen["n_bank"] and set(RB.POINTS) <= seen["pts"]
    assert set(RB.SHIFTS) <= seen["n_tau"] and seen["h_ld"] == {2, 4} and seen["weighted"] == {True, False}
    assert RB.ROWS == (1, 15, 16, 17, 33) and RB.BANKS == (1, 15, 16, 17, 40) and RB.POINTS == (1, 2, 3, 5, 127, 128, 129, 200)
    assert RB.SHIFTS == (0, 1, 15, 16, 17, 33)


def test_column_g_equals_the_match_reference_on_template_g_broadcast_over_the_tasks(all_cases):
    worst = 0.0
    for tag, fac, case, ref in all_cases:
        if fac["n_rows"] * fac["n_bank"] > 200:
            continue  # (the sweeps: every path of the reference; the one large case adds nothing to this check)
        for g in range(fac["n_bank"]):
            one = M.reference(case["h"], case["bank"][g:g + 1], case["weights"], case["freqs"], case["taus"])
            for name in ("match", "mismatch", "phase"):
                d = float((one[name] - ref[name][:, g]).abs().max())
                worst = max(worst, d)
                assert d <= 1e-12, (tag, g, name, d)
            assert torch.equal(one["tau_index"], ref["tau_index"][:, g]), (tag, g)
            assert float((one["hh"] - ref["hh"]).abs().max()) <= 1e-12 * float(ref["hh"].abs().max()), (tag, g)
            assert abs(float(one["gg"][0] - ref["gg"][g])) <= 1e-12 * float(ref["gg"][g].abs()), (tag, g)
            assert float((one["corr"].pow(2).sum(-1).sqrt() - ref["mag"][:, g]).abs().max()) <= 1e-12, (tag, g)
    print(f"BANK reference column against match_reference: worst difference {worst:.3g}")


def test_every_case_leaves_tau_index_and_best_index_well_posed(all_cases):
    worst_j, worst_g = math.inf, math.inf
    for tag, fac, case, ref in all_cases:
        assert not ref["degenerate"].any() and torch.isfinite(ref["match"]).all(), tag
        if ref["mag"].shape[2] >= 2:
            top = ref["mag"].topk(2, dim=2).values
            gap = float((top[..., 0] - top[..., 1]).min())
            worst_j = min(worst_j, gap)
            assert gap >= 1e-6, f"{tag}: the runner-up of max_j |c_j| lies {gap:.3g} below the best"
        if fac["n_bank"] >= 2:
            top = ref["match"].topk(2, dim=1).values
            gap = float((top[:, 0] - top[:, 1]).min())
            worst_g = min(worst_g, gap)
            assert gap >= 1e-6, f"{tag}: the runner-up template lies {gap:.3g} below best_match"
        assert (ref["match"] <= 1.0 + 1e-12).all(), tag  # Cauchy-Schwarz
    print(f"BANK smallest runner-up margin over the cases: shifts {worst_j:.3g}, templates {worst_g:.3g}")


def test_the_planted_template_and_shift_are_found(all_cases):
    for tag, fac, case, ref in all_cases:
        if fac["pts"] < 100:
            continue  # (a few points cannot tell chirps apart)
        r = torch.arange(fac["n_rows"])
        assert torch.equal(ref["best_index"], (5 * r + 2) % fac["n_bank"]), tag
        if fac["n_tau"]:
            assert torch.equal(ref["tau_index"][r, ref["best_index"]], (3 * r + 1) % fac["n_tau"]), tag
