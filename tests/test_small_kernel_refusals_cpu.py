"""CPU: the small kernels' entry points refuse what their vector accesses and 32-bit indices cannot serve -- operands off a 16-byte
boundary, strides narrower than the width, h * w or rows * dim / 2 beyond 32 bits -- with TT_EINVAL, before any launch.  One valid
argument set per entry point with one fault at a time (tests/small_kernel_refusals.py), answered in a child process that sees no GPU."""
import pytest

from tests.small_kernel_refusals import ENTRIES, ROWS, TT_EINVAL, row_id, run_child

IDS = [row_id(e, f) for e, f in ROWS]


@pytest.fixture(scope="module")
def answers():
    return run_child()


def test_every_entry_point_has_rows():
    assert len(set(IDS)) == len(IDS) and {e for e, _ in ROWS} == set(ENTRIES)


@pytest.mark.parametrize("entry,fault", ROWS, ids=IDS)
def test_refusal(answers, entry, fault):
    code, message, untouched = answers[row_id(entry, fault)]
    assert code == TT_EINVAL, (code, message)
    assert message.startswith(entry + ":"), message
    assert untouched, "the output buffer was written"
