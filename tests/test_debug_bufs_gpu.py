"""The unit-test hooks' common device staging (csrc/debug_bufs.h) checked on itself: vrag_debug_canary_selftest stages three
small buffers the way every hook does, launches nothing, and lets a host-issued one-byte hipMemset land inside buffer "b"'s
own allocation.  The canary check must fire on the first and on the last canary byte and name the buffer; it must stay quiet
when nothing is touched and when the byte lies in the pad in front of the canary, and "b" must come back as it went in."""
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib

gpu = pytest.mark.gpu
OK, ERR_INVALID, ERR_HIP = 0, -1, -2


def selftest(touch, device=0):
    dbg = _lib.load_debug()
    status = dbg.vrag_debug_canary_selftest(touch, device)
    msg = dbg.vrag_last_error()
    return status, msg.decode("utf-8", "replace") if msg else ""


@pytest.mark.parametrize("touch", [-1, 4, 1 << 20])
def test_unknown_touch_is_refused_before_the_device_check(touch):
    """No device is looked for: device 1 << 20 would be VRAG_ERR_NO_DEVICE (-4), and the call needs no GPU."""
    status, msg = selftest(touch, device=1 << 20)
    assert status == ERR_INVALID and "touch" in msg


@gpu
@pytest.mark.parametrize("touch", [-1, 4])
def test_unknown_touch_is_refused_on_a_device_too(touch):
    assert selftest(touch)[0] == ERR_INVALID


@gpu
@pytest.mark.parametrize("touch", [0, 3])
def test_untouched_canaries_and_a_written_pad_byte_pass(touch):
    """touch 0 also checks inside the hook that b's 100 bytes came back unchanged (the host copy is cleared after staging)."""
    status, msg = selftest(touch)
    assert status == OK, msg


@gpu
@pytest.mark.parametrize("touch", [1, 2])
def test_first_and_last_canary_byte_fire_and_name_the_buffer(touch):
    status, msg = selftest(touch)
    assert status == ERR_HIP
    assert msg == "debug canary selftest run: the launch wrote past the end of b"
