"""CPU: the guarded arenas of tests/arena.py can fail. Each defect the output-contract tests
(tests/test_gpu_contracts.py) exist to catch is planted on a CPU arena and must be reported
with its position; a clean run must report nothing."""
import pytest
import torch

from arena import GUARD, POISONS, Arena, arena

CPU = torch.device("cpu")
SPECS = [100, 0, (5, 7, torch.float32), (5, 7, torch.float32, 10), (3, 16, torch.uint8, 17),
         (1, 2, torch.int32), (0, 16, torch.float32), (67, 3, torch.float32, 6)]


def ids(s):
    return str(s).replace("torch.", "")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("spec", SPECS, ids=ids)
def test_layout_and_clean_run(spec, poison):
    a = arena(spec, CPU, poison)
    assert a.buf.numel() == 2 * GUARD + a.nbytes and a.ptr == a.buf.data_ptr() + GUARD
    assert a.ptr % 16 == a.buf.data_ptr() % 16          # the payload keeps the alignment
    if a.nbytes:
        assert a.payload.data_ptr() == a.ptr
        r, c = (a.rows - 1, a.cols - 1)
        last = a.payload[c] if isinstance(spec, int) else a.payload[r, c]
        assert last.data_ptr() + a.itemsize == a.ptr + a.nbytes   # no rounding before the guard
    assert a.check() is None
    if a.nbytes:
        assert a.first_poisoned() == ((0,) if isinstance(spec, int) else (0, 0))
    a.payload.zero_()                                    # a kernel that writes every element
    assert a.check() is None and a.first_poisoned() is None
    assert bool((a.buf[:GUARD] == poison).all()) and bool((a.buf[GUARD + a.nbytes:] == poison).all())


def test_poison_patterns_read_as_documented():
    nan = arena((1, 4, torch.float32), CPU, 0xFF).payload
    assert bool(torch.isnan(nan).all())
    assert arena((1, 4, torch.int32), CPU, 0xFF).payload.tolist() == [[-1] * 4]
    big = arena((1, 4, torch.float32), CPU, 0x5A).payload
    assert bool(torch.isfinite(big).all()) and 1e16 < float(big[0, 0]) < 2e16


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("spec", SPECS, ids=ids)
def test_byte_before_the_payload_is_reported(spec, poison):
    a = arena(spec, CPU, poison)
    a.payload.zero_()
    a.buf[GUARD - 1] = poison ^ 0x01
    assert a.check() == ("leading guard", -1, poison ^ 0x01)
    a.buf[7] = 0
    assert a.check() == ("leading guard", 7 - GUARD, 0)  # the first changed byte


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("spec", SPECS, ids=ids)
def test_byte_after_the_payload_is_reported(spec, poison):
    a = arena(spec, CPU, poison)
    a.payload.zero_()
    a.buf[GUARD + a.nbytes] = 0
    assert a.check() == ("trailing guard", a.nbytes, 0)
    a = arena(spec, CPU, poison)
    a.buf[-1] = 1                                         # the far end of the guard
    assert a.check() == ("trailing guard", a.nbytes + GUARD - 1, 1)


@pytest.mark.parametrize("poison", POISONS)
def test_byte_in_a_stride_gap_is_reported(poison):
    a = arena((5, 7, torch.float32, 10), CPU, poison)
    a.payload.zero_()
    assert a.check() is None
    # row 3's gap: floats 3 * 10 + 7 .. 3 * 10 + 9; its second float's third byte
    pos = (3 * 10 + 8) * 4 + 2
    a.buf[GUARD + pos] = 0
    assert a.check() == ("gap after row 3", pos, 0)
    # a vector store that runs over the row's end: the first gap byte is the one reported
    b = arena((3, 16, torch.uint8, 17), CPU, poison)
    b.payload.zero_()
    b.buf[GUARD + 16:GUARD + 17] = 0
    assert b.check() == ("gap after row 0", 16, 0)
    # the last row has no gap: the byte behind it is the trailing guard
    b = arena((3, 16, torch.uint8, 17), CPU, poison)
    b.buf[GUARD + 2 * 17 + 16] = 0
    assert b.check() == ("trailing guard", b.nbytes, 0)


@pytest.mark.parametrize("poison", POISONS)
def test_unwritten_payload_element_is_reported(poison):
    a = arena((5, 7, torch.float32, 10), CPU, poison)
    a.payload.zero_()
    a.payload.view(torch.int32)[4, 6] = int.from_bytes(bytes([poison] * 4), "little", signed=True)
    assert a.first_poisoned() == (4, 6) and a.check() is None
    # and it fails the two bars of the contract tests: bit equality and the relative bound
    assert not torch.equal(a.payload.view(torch.int32), torch.zeros(5, 7, dtype=torch.int32))
    err = (a.payload.double() - 0.0).abs()
    assert not bool((err <= 1e-5).all())                  # NaN compares false, 1.5e16 is far off
    c = arena(12, CPU, poison)
    c.payload[:11] = 0
    assert c.first_poisoned() == (11,)
    one = Arena((2, 2, torch.int32), CPU, poison)
    one.payload[0, 0] = 5
    assert one.first_poisoned() == (0, 1)


def test_fill_sets_a_prior_and_keeps_the_guards():
    a = arena((3, 4, torch.float32, 6), CPU, 0xFF)
    prior = torch.arange(12, dtype=torch.float32).view(3, 4)
    a.fill(prior)
    assert torch.equal(a.payload, prior) and a.check() is None and a.first_poisoned() is None
