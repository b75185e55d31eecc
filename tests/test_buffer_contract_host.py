"""tests/buffer_contract.py must see every fault it exists for.  The "kernels" here are torch CPU ops that commit one
fault each on a guard-banded buffer; a correct writer must pass, at both base offsets and every element type."""

import numpy as np
import pytest
import torch

from buffer_contract import GUARD_BYTES, SENTINEL_BITS, ContractViolation, guarded

DTYPES = [torch.float64, torch.float32, torch.int64]
ROWS, COLS, LD = 5, 7, 10  # an output of 7 documented columns in rows LD = 10 apart: columns 7..9 are pad


def _written_mask():
    m = np.zeros((ROWS, LD), dtype=bool)
    m[:, :COLS] = True
    return m


def _values(dtype, shape):
    v = torch.arange(1, int(np.prod(shape)) + 1).reshape(shape)
    return v.to(dtype)


def correct_writer(out):
    out[:, :COLS] = _values(out.dtype, (ROWS, COLS))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [0, 1])
def test_layout_and_a_correct_writer(dtype, offset):
    out, chk = guarded((ROWS, LD), dtype, offset)
    esize = out.element_size()
    assert out.data_ptr() % 16 == (offset * esize) % 16 and out.is_contiguous() and out.shape == (ROWS, LD)
    assert chk.guard * esize >= GUARD_BYTES and chk.flat.numel() == 2 * chk.guard + offset + ROWS * LD
    assert bool((chk.flat.view(torch.int64 if esize == 8 else torch.int32) == SENTINEL_BITS[dtype]).all())
    if dtype != torch.int64:
        assert bool(torch.isnan(out).all())  # a float sentinel that is read early poisons the result
    else:
        assert bool((out < 0).all())
    correct_writer(out)
    chk.check_output(_written_mask())
    inp, ichk = guarded((ROWS, COLS), dtype, offset)
    ichk.upload(_values(dtype, (ROWS, COLS)))
    _ = inp.sum()
    ichk.check_input()


def _flat_index(chk, payload_elem):
    return chk.start + payload_elem


FAULTS = ["past_end", "before_start", "unwritten", "pad_column", "far_guard"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("fault", FAULTS)
def test_every_output_fault_is_seen(dtype, offset, fault):
    out, chk = guarded((ROWS, LD), dtype, offset)
    correct_writer(out)
    one = torch.ones((), dtype=dtype)
    if fault == "past_end":
        chk.flat[_flat_index(chk, ROWS * LD)] = one
    elif fault == "before_start":
        chk.flat[_flat_index(chk, -1)] = one  # with offset 1 this is the pad element
    elif fault == "unwritten":
        chk.flat.view(torch.int64 if out.element_size() == 8 else torch.int32)[_flat_index(chk, 2 * LD + 3)] = \
            SENTINEL_BITS[dtype]
    elif fault == "pad_column":
        out[ROWS - 1, COLS] = one
    elif fault == "far_guard":
        chk.flat[-1] = one  # the last element of the 64 KiB band
    with pytest.raises(ContractViolation):
        chk.check_output(_written_mask())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [0, 1])
def test_an_input_scaled_in_place_or_overrun_is_seen(dtype, offset):
    inp, chk = guarded((ROWS, COLS), dtype, offset)
    chk.upload(_values(dtype, (ROWS, COLS)))
    inp.mul_(2)  # a kernel that normalises its argument in place
    with pytest.raises(ContractViolation):
        chk.check_input()
    inp2, chk2 = guarded((ROWS, COLS), dtype, offset)
    chk2.upload(_values(dtype, (ROWS, COLS)))
    chk2.flat[chk2.start - 1 - offset] = 1  # a write into the leading guard of an input
    with pytest.raises(ContractViolation):
        chk2.check_input()


def test_a_nan_result_counts_as_written_and_a_late_fill_is_expected():
    out, chk = guarded((4,), torch.float64, 1)
    out.copy_(torch.tensor([1.0, float("nan"), 0.0, -0.0]).double())  # the arithmetic NaN is not the sentinel
    chk.check_output()
    inp, ichk = guarded((3,), torch.float32, 1)
    vals = torch.tensor([1.0, 2.0, 3.0])
    ichk.expect(vals)
    with pytest.raises(ContractViolation):  # not filled yet
        ichk.check_input()
    inp.copy_(vals)
    ichk.check_input()


def test_written_nothing_and_whole_regions():
    out, chk = guarded((3, 4), torch.float64, 0)
    chk.check_output(np.zeros((3, 4), dtype=bool))  # the "writes nothing" contract of an empty call
    with pytest.raises(ContractViolation):
        chk.check_output()  # ... and not the full-write one
    out.zero_()
    chk.check_output()
    with pytest.raises(ContractViolation):
        chk.check_output(np.zeros((3, 4), dtype=bool))
