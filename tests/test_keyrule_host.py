"""Host side of the key rules (CPU, no kernel launched): ``live()`` of each of the five rules against the expression it stands for,
worked out here in plain Python, and ``as_key_rule``.  (``functional.key_weights(detach=...)`` is not reached on a CPU tensor: its
device refusal comes first and is pinned by test_keyweight_host.py / test_reweight_host.py.)"""
import math

import pytest
import torch

from npf_gwwaveform_amd.architectures import FirstKeys, KeyRule, KeyWeights, LeaveOneOut, PrefixTail, TrainKeyWeights, as_key_rule

C = 4
COUNTS = [0, 1, 2, C, C + 3, -1]
NAN, INF = float("nan"), float("inf")
# (one row per count: nothing below a count of 0; the only positive weight beyond the count; a positive weight below it among a
# negative one and zeros; 0 / negative / NaN / Inf only; one positive weight among those under a count beyond C; a negative count)
WEIGHTS = [[1.0, 1.0, 1.0, 1.0], [0.0, 2.0, 2.0, 2.0], [-1.0, 0.5, 0.0, 0.0], [NAN, INF, 0.0, -2.0], [NAN, INF, 0.0, 3.0],
           [1.0, 1.0, 1.0, 1.0]]


def _admissible(rows, counts):
    return [any(k < n and 0 < w < INF and not math.isnan(w) for k, w in enumerate(row)) for row, n in zip(rows, counts)]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_count_rules_are_live_where_a_key_is_left(dtype):
    n = torch.tensor(COUNTS, dtype=dtype)
    assert FirstKeys(n).live(len(COUNTS)).tolist() == [c > 0 for c in COUNTS] == [False, True, True, True, True, False]
    assert LeaveOneOut(n).live(len(COUNTS)).tolist() == [c > 1 for c in COUNTS] == [False, False, True, True, True, False]
    assert FirstKeys(n).live(len(COUNTS)).dtype == torch.bool


def test_train_key_weights_are_live_where_a_key_is_admissible():
    n = torch.tensor(COUNTS, dtype=torch.int32)
    w = torch.tensor(WEIGHTS, requires_grad=True)
    live = TrainKeyWeights(w, n).live(len(COUNTS))
    assert live.tolist() == _admissible(WEIGHTS, COUNTS) == [False, False, True, False, True, False]
    assert live.dtype == torch.bool and not live.requires_grad


def test_key_weights_are_live_per_replicate():
    n = torch.tensor(COUNTS, dtype=torch.int32)
    flipped = [row[::-1] for row in WEIGHTS]  # (the second replicate: what lay beyond a count now lies below it, and the reverse)
    live = KeyWeights(torch.tensor([WEIGHTS, flipped]), n, 2).live(2 * len(COUNTS))
    assert live.tolist() == _admissible(WEIGHTS + flipped, COUNTS + COUNTS)
    assert live.tolist()[len(COUNTS):] == [False, True, False, False, True, False]


def test_prefix_tail_is_live_where_either_segment_has_a_row():
    m_tail, S = 3, 2
    n_tail = [0, 0, 0, 0, 0, 0, 0, -1, 1, m_tail + 2, -5, 2]
    rule = PrefixTail(None, None, torch.tensor(COUNTS, dtype=torch.int32), None, None, torch.tensor(n_tail, dtype=torch.int32),
                      len(COUNTS), C, m_tail)
    want = [min(max(p, 0), C) + min(max(t, 0), m_tail) > 0 for p, t in zip(COUNTS * S, n_tail)]
    assert rule.live(S * len(COUNTS)).tolist() == want
    assert want == [False, True, True, True, True, False, False, True, True, True, True, True]


def test_as_key_rule_wraps_a_tensor_and_passes_rules_through():
    n = torch.tensor(COUNTS, dtype=torch.int32)
    wrapped = as_key_rule(n)
    assert type(wrapped) is FirstKeys and wrapped.n_valid is n
    w = torch.tensor(WEIGHTS)
    for rule in (wrapped, LeaveOneOut(n), KeyWeights(w.unsqueeze(0), n, 1), TrainKeyWeights(w, n),
                 PrefixTail(None, None, n, None, None, n, len(COUNTS), C, 3)):
        assert isinstance(rule, KeyRule) and as_key_rule(rule) is rule
