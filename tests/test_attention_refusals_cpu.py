"""CPU: tt_attention and tt_temporal_attention refuse what they refused before -- same order of checks, same return codes, same messages.  One valid
argument set per family with one fault at a time (tests/attention_refusals.py), answered by the library under test in a child process
that sees no GPU, against the codes recorded from the parent commit's library (tests/golden/attention_refusals.json)."""
import json
import os

import pytest

from tests.attention_refusals import ATTENTION_ROWS, TEMPORAL_ROWS, row_id, run_child

IDS = [row_id(f, fault) for f, fault in ATTENTION_ROWS] + [row_id("temporal", fault) for fault in TEMPORAL_ROWS]

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_refusals.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def answers():
    return run_child()


def test_the_fixture_covers_exactly_the_rows():
    assert sorted(GOLDEN) == sorted(IDS) and len(set(IDS)) == len(IDS)
    assert {code for code, _ in GOLDEN.values()} <= {-1, -2}                   # TT_EINVAL / TT_EUNSUPPORTED: no row ever reached a launch


@pytest.mark.parametrize("row", IDS)
def test_refusal_code(answers, row):
    assert answers[row] == GOLDEN[row]
