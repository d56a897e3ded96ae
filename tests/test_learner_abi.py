"""CPU tests that the fused learner updates keep what they show through the C ABI: every workspace size and every refusal (return
code and message) equals the record in tests/golden/learner_abi.json (tests/learner_abi.py, tests/golden/gen_learner_abi.py)."""
import pytest

import learner_abi
from conftest import golden_json


@pytest.fixture(scope="module")
def now():
    return learner_abi.record()


@pytest.mark.parametrize("algo", sorted(learner_abi.ALGOS))
def test_workspace_sizes_equal_the_record(now, algo):
    """all of state_dim 0..13 x hidden_dim {128, 256} x 17 batch sizes, the -1 answers included"""
    want, have = golden_json("learner_abi.json")["sizes"][algo], now["sizes"][algo]
    assert len(want) == len(learner_abi.STATE_DIMS) * len(learner_abi.HIDDEN_DIMS) * len(learner_abi.BATCHES)
    assert [r for r in have if r not in want] == [] and have == want
    assert sum(1 for r in want if r[3] > 0) == 12 * 15 and all(r[3] == -1 or r[3] > 0 for r in want)


@pytest.mark.parametrize("algo", sorted(learner_abi.ALGOS))
def test_refusals_equal_the_record(now, algo):
    """every mutation of the host tests' lists and a NULL args: the same return code and the same message, byte for byte"""
    want, have = golden_json("learner_abi.json")["refusals"][algo], now["refusals"][algo]
    assert len(want) >= 13 and want[-1][0] == "NULL args"
    for w, h in zip(want, have):
        assert h == w
    assert len(have) == len(want)
