"""Host / device parity of the engine wrappers: every wrapper of scri_amd/engine.py that takes a numpy array or a device tensor is
called on the same values in host memory, in contiguous device memory and, where it takes a row stride, on a column slice of a wider
device tensor (tests/helpers/abi_cases.py).  Every output of the three calls is compared bit for bit: a host array goes through the
same launches as a device tensor, so how an argument is staged must not show in a result.

Cases held to a tolerance instead of equal bits: none."""
import numpy as np
import pytest

from tests.helpers import abi_cases

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", abi_cases.CASES, ids=abi_cases.IDS)
def test_host_and_device_give_the_same_bits(ctx, case):
    expect = case.run(ctx, "host")
    assert expect, "a case has outputs"
    for layout in case.layouts[1:]:
        got = case.run(ctx, layout)
        assert len(got) == len(expect)
        for k, (g, e) in enumerate(zip(got, expect)):
            assert _same_bits(g, e), f"{case.id}: output {k} of the {layout} call differs from the host call's:\n{g}\n{e}"
