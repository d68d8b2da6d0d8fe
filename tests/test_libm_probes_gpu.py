"""The probe lenses of tests/libm_probes.py on the DEVICE: one hiprtc compile and one launch of a few thousand threads per probe.

Values: what the generated code computes on the device equals, bit for bit (NaN beside NaN, result counts and error bits included), what
the host interpreter computes on the portable libm - and the libm columns equal libbkm_host.so directly, which makes the comparison
"device build of bkm.h == host build of bkm.h", with mpmath behind the host build (tests/test_bkm.py).  Over whole domains: the seams of
the reductions, overflow and underflow, subnormals, the C99 special cases, conversion edges, +-0 / +-inf / NaN in every position.

Bounds and flags: every CPU exactness test runs the generated code under tests/hostemu; that vouches for the GPU only if the device
computes the same bound e and the same flag.  bk_debug_eval_device_bounds makes them visible: (value, bound, flag, result count, error
bits) on the device equal hostemu's bit for bit, at the default BK_LIBM_REL and at 2^-30."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostemu"))

import libm_probes as LP     # noqa: E402

pytestmark = pytest.mark.gpu

_inputs = {}


def wide():
    if "wide" not in _inputs:
        _inputs["wide"] = LP.wide_inputs()
        _inputs["wide"].setflags(write=False)
    return _inputs["wide"]


def device_equals_interpreter(name, body, refs, args):
    import blinky_amd as bk
    ctx = LP.make_context(bk, LP.lens(body), "probe_" + name, device=0)
    d_out, d_n = ctx.eval_device(1, args)
    h_out, h_n = LP.eval_host_errs(bk, ctx, 1, args)
    ctx.close()
    ok = d_n == h_n
    assert ok.all(), f"{name}: result count / error bits, device vs interpreter: " + LP.first_mismatch(ok, args, d_n, h_n)
    ran = h_n >= 0
    for k in range(8):
        ok = LP.same_bits(d_out[:, k], h_out[:, k]) | ~ran
        assert ok.all(), f"{name} column {k}, device vs interpreter: " + LP.first_mismatch(ok, args, d_out[:, k], h_out[:, k])
    for k, ref in enumerate(refs):
        if ref is None:
            continue
        want = ref(args)
        ok = LP.same_bits(d_out[:, k], want) | ~ran
        assert ok.all(), f"{name} column {k}, device vs libbkm_host / the Lua 5.2 definition: " + LP.first_mismatch(ok, args, d_out[:, k], want)
    return d_out, d_n


@pytest.mark.parametrize("name", sorted(LP.VALUE_PROBES))
def test_value_probes_device_equals_interpreter_and_host_bkm(name):
    body, refs = LP.VALUE_PROBES[name]
    device_equals_interpreter(name, body, refs, wide())


def test_plate_to_ray_of_an_index_outside_the_globe_is_nil_on_the_device():
    """a NaN plate index is INT_MIN to the reference's conversion and 0 to the GPU's own: nil, like every index outside the six plates"""
    import blinky_amd as bk
    args, valid = LP.plate_nil_inputs()
    ctx = LP.make_context(bk, LP.lens(LP.PLATE_NIL_PROBE), "plate_nil", device=0)
    d_out, d_n = ctx.eval_device(1, args)
    ctx.close()
    assert (d_n == 1).all() and d_out[:, 0].tolist() == np.where(valid, 0.0, 3.0).tolist()


def test_control_probe_device_equals_interpreter():
    args = LP.control_inputs()
    d_out, d_n = device_equals_interpreter("control", LP.CONTROL_PROBE, [None] * 3, args)
    assert d_n[-1] == -100 - LP.ERR_LOOP and (d_n[:-1] == 3).all()


BOUND_CASES = ([(n, b, None) for n, b in sorted(LP.BOUND_PROBES.items())] + [("x_" + n, b, t) for n, (b, t) in sorted(LP.EXTREME_PROBES.items())] +
               [("exact", LP.EXACT_PROBE, None)])


@pytest.mark.parametrize("rel_log2", [0, 30], ids=["default", "2^-30"])
@pytest.mark.parametrize("case", BOUND_CASES, ids=[c[0] for c in BOUND_CASES])
def test_device_bounds_and_flags_equal_the_host_emulation(case, rel_log2, request):
    if not (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")):
        pytest.skip("no host C++ compiler on this box (tests/hostemu)")
    import blinky_amd as bk
    import emu
    name, body, found_at = case
    args = wide() if not found_at else np.concatenate([np.array(found_at, np.float64).reshape(-1, 3), wide()])
    bk.debug_set_option("libm_rel_log2", rel_log2)
    request.addfinalizer(lambda: bk.debug_set_option("libm_rel_log2", 0))
    ctx = LP.make_context(bk, LP.lens(body), "bound_" + name, device=0)
    d_out, d_bound, d_flag, d_n = ctx.eval_device_bounds(1, args)
    ctx.close()
    bk.debug_set_option("libm_rel_log2", 0)
    host = LP.make_context(bk, LP.lens(body), "bound_" + name)                     # (device-less, as every hostemu test has it)
    dev = emu.forward_values(host, args, defines=("BK_LIBM_REL=0x1p-30",) if rel_log2 else ())
    host.close()
    used = (np.arange(8)[None, :] < dev["nret"][:, None]) & (dev["tag"] == 3)
    e_out, e_bound = np.where(used, dev["val"], np.nan), np.where(used, dev["bound"], 0.0)
    e_n = np.where(dev["err"] != 0, -100 - dev["err"], dev["nret"]).astype(np.int32)
    ok = d_n == e_n
    assert ok.all(), f"{name}: result count / error bits, device vs hostemu: " + LP.first_mismatch(ok, args, d_n, e_n)
    ok = d_flag == dev["flag"]
    assert ok.all(), f"{name}: flag, device vs hostemu: " + LP.first_mismatch(ok, args, d_flag, dev["flag"])
    for k in range(8):
        ok = LP.same_bits(d_out[:, k], e_out[:, k])
        assert ok.all(), f"{name} column {k}: value, device vs hostemu: " + LP.first_mismatch(ok, args, d_out[:, k], e_out[:, k])
        ok = LP.same_bits(d_bound[:, k], e_bound[:, k])
        assert ok.all(), f"{name} column {k}: bound, device vs hostemu: " + LP.first_mismatch(ok, args, d_bound[:, k], e_bound[:, k])
    if name == "exact":
        assert not d_flag.any() and (d_bound.view(np.uint64) == 0).all()
    elif name in LP.BOUND_PROBES:
        # the bookkeeping is alive on the device.  Only the ordinary probes promise that: the extreme group may flag everything it
        # computes (found_subnormal does: every result is subnormal, so every bound it returns is the 0 of a flagged value)
        assert (d_bound > 0).any() and (d_flag != 0).any() and (d_flag == 0).any()
