"""The probe lenses of tests/libm_probes.py WITHOUT a GPU.

Values: the host interpreter on the portable libm, the generated code under tests/hostemu and libbkm_host.so must agree bit for bit over
whole domains - the seams of bkm.h's reductions, overflow and underflow, subnormals, the C99 special cases, conversion edges, +-0 / +-inf /
NaN in every argument position - and the runtime operators must be the Lua 5.2 definitions.  (tests/test_libm_probes_gpu.py then holds the
device against the same interpreter and the same library.)

Bounds: every value the generated code computes from an inexact one carries a bound; on a stand-in libm 2^-30 away from bkm.h the host
interpreter must land within it wherever the generated code did not raise the flag - here on composites of every family of operations,
and on values scaled through the subnormal range and towards overflow, where the shipped lenses never go."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostemu"))

import emu                                      # noqa: E402
import libm_probes as LP                        # noqa: E402
from test_exactness_cpu import check_bounds    # noqa: E402

_inputs = {}


def wide():
    """the shared input set, built once and never written to"""
    if "wide" not in _inputs:
        _inputs["wide"] = LP.wide_inputs()
        _inputs["wide"].setflags(write=False)
    return _inputs["wide"]


def emu_as_device(dev):
    """emu.forward_values' answer in the form bk_debug_eval_device gives: (out [n, 8] with NaN for everything that is not a returned
    number, nout with -100 - err for a run-time error)"""
    used = (np.arange(8)[None, :] < dev["nret"][:, None]) & (dev["tag"] == 3)
    out = np.where(used, dev["val"], np.nan)
    nout = np.where(dev["err"] != 0, -100 - dev["err"], dev["nret"]).astype(np.int32)
    return out, nout


def values_three_ways(name, body, refs, args):
    import blinky_amd as bk
    ctx = LP.make_context(bk, LP.lens(body), "probe_" + name)
    h_out, h_n = LP.eval_host_errs(bk, ctx, 1, args)
    dev = emu.forward_values(ctx, args)
    ctx.close()
    e_out, e_n = emu_as_device(dev)
    np.testing.assert_array_equal(e_n, h_n)
    ran = h_n >= 0                                                   # (after a run-time error there is no result to compare)
    for k in range(8):
        ok = LP.same_bits(e_out[:, k], h_out[:, k]) | ~ran
        assert ok.all(), f"{name} column {k}, hostemu vs interpreter: " + LP.first_mismatch(ok, args, e_out[:, k], h_out[:, k])
    for k, ref in enumerate(refs):
        if ref is None:
            continue
        assert (h_n[ran] > k).all()
        want = ref(args)
        ok = LP.same_bits(h_out[:, k], want) | ~ran
        assert ok.all(), f"{name} column {k}, interpreter vs reference: " + LP.first_mismatch(ok, args, h_out[:, k], want)
    return h_out, h_n


@pytest.mark.parametrize("name", sorted(LP.VALUE_PROBES))
def test_value_probes_interpreter_hostemu_and_bkm_agree(name):
    body, refs = LP.VALUE_PROBES[name]
    h_out, h_n = values_three_ways(name, body, refs, wide())
    assert (h_n == len(refs)).all()


def test_plate_to_ray_of_an_index_outside_the_globe_is_nil():
    """NaN beside NaN cannot tell nil from a NaN number, so the probe counts the nils itself.  A plate index that is NaN, negative, past the last plate or
    outside int gives nil on both sides - a NaN index truncates to INT_MIN in the reference, not to plate 0"""
    import blinky_amd as bk
    args, valid = LP.plate_nil_inputs()
    assert valid.tolist() == [False, False, False, False, True, True, True, True, False, False, False, False, False, False, True]
    ctx = LP.make_context(bk, LP.lens(LP.PLATE_NIL_PROBE), "plate_nil")
    dev = emu.forward_values(ctx, args)
    host = [ctx.eval_host(1, *[float(v) for v in a]) for a in args]
    ctx.close()
    assert (dev["err"] == 0).all() and (dev["flag"] == 0).all() and (dev["nret"] == 1).all() and (dev["tag"][:, 0] == 3).all()
    want = np.where(valid, 0.0, 3.0).tolist()
    assert dev["val"][:, 0].tolist() == want
    assert [r[0] for r in host] == want


def test_control_probe_table_index_and_loop_bounds_from_the_arguments():
    args = LP.control_inputs()
    h_out, h_n = values_three_ways("control", LP.CONTROL_PROBE, [None] * 3, args)
    # the table: t[x] for x = 1..4 exactly, nothing (the `or -1`) for every other index
    ran = h_n == 3
    x = args[ran, 0]
    want = np.where((x == 1) | (x == 2) | (x == 3) | (x == 4), 10 * x, -1.0)
    np.testing.assert_array_equal(h_out[ran, 0], want)
    # the loop: counts of the ordinary tuples, and the budget on those that run away
    assert (h_n[-1:] == -100 - LP.ERR_LOOP).all(), h_n[-1:]
    assert (h_n[:-1] == 3).all()
    lim, step = args[:-1, 1], args[:-1, 2]
    fin = np.isfinite(lim) & np.isfinite(step) & (step > 0)
    with np.errstate(all="ignore"):
        count = np.where(lim >= 1, np.floor((lim - 1) / step) + 1, 0)
    np.testing.assert_array_equal(h_out[:-1, 2][fin], count[fin])


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
MODES = [(30, "random"), (30 + 64, "all-high"), (30 + 128, "all-low")]
_emu_cache = {}


def bound_probe_values(name, body, args):
    """the generated code's (value, bound, flag) at BK_LIBM_REL = 2^-30: computed once per probe, shared by the three modes"""
    import blinky_amd as bk
    if name not in _emu_cache:
        ctx = LP.make_context(bk, LP.lens(body), "bound_" + name)
        _emu_cache[name] = emu.forward_values(ctx, args, defines=("BK_LIBM_REL=0x1p-30",))
        ctx.close()
    return _emu_cache[name]


def run_check_bounds(name, body, args, mode):
    import blinky_amd as bk
    dev = bound_probe_values(name, body, args)
    ctx = LP.make_context(bk, LP.lens(body), "bound_" + name, host_math=mode)
    try:
        check_bounds(ctx, 1, dev, args, range(len(args)), f"{name}/{mode}")
    finally:
        ctx.close()
    return dev


@pytest.mark.parametrize("mode", [m for m, _ in MODES], ids=[i for _, i in MODES])
@pytest.mark.parametrize("name", sorted(LP.BOUND_PROBES))
def test_bound_probes_hold_against_an_adversarial_libm(name, mode):
    args = wide()
    dev = run_check_bounds(name, LP.BOUND_PROBES[name], args, mode)
    # the check must not be vacuous: most tuples are decided on the device, and every column is checked a thousand times over
    flagged = dev["flag"] != 0
    assert (dev["err"] == 0).all()
    assert flagged.mean() <= 0.25, f"{name}: {flagged.mean():.3f} of the tuples are flagged"
    nret = int(dev["nret"].max())
    for k in range(nret):
        checked = (~flagged) & (dev["nret"] > k) & (dev["tag"][:, k] == 3) & np.isfinite(dev["val"][:, k])
        assert checked.sum() >= 1000, f"{name} column {k}: {int(checked.sum())} checked finite values"


@pytest.mark.parametrize("mode", [m for m, _ in MODES], ids=[i for _, i in MODES])
@pytest.mark.parametrize("name", sorted(LP.EXTREME_PROBES))
def test_extreme_probes_hold_against_an_adversarial_libm(name, mode):
    """values scaled through the subnormal range and towards overflow (flags are free here: a flag is the safe answer), the tuples that
    found the three holes first"""
    body, found_at = LP.EXTREME_PROBES[name]
    args = np.concatenate([np.array(found_at, np.float64).reshape(-1, 3), wide()])
    run_check_bounds(name, body, args, mode)


def test_exact_arithmetic_through_the_subnormal_range_is_never_flagged():
    """the same scalings on exact arguments (no libm call upstream) stay the device's business: no flag, every bound exactly 0"""
    import blinky_amd as bk
    args = wide()
    ctx = LP.make_context(bk, LP.lens(LP.EXACT_PROBE), "exact")
    h_out, h_n = LP.eval_host_errs(bk, ctx, 1, args)
    for defines in ((), ("BK_LIBM_REL=0x1p-30",)):
        dev = emu.forward_values(ctx, args, defines=defines)
        assert (dev["flag"] == 0).all(), f"{int((dev['flag'] != 0).sum())} tuples of exact arithmetic flagged"
        assert (dev["err"] == 0).all() and (dev["nret"] == 8).all() and (h_n == 8).all()
        assert (dev["bound"].view(np.uint64) == 0).all(), "a bound on exact arithmetic"
        assert LP.same_bits(dev["val"], h_out).all()
    ctx.close()
    assert np.isfinite(h_out).any(axis=0).all() and ((h_out != 0) & (np.abs(h_out) < 2.3e-308)).any()     # (subnormal results do occur)


def test_the_emitter_names_its_two_limits_on_return_values():
    """eight values, or four in front of a trailing call (why the probes return through locals): each refusal says which limit it is"""
    import blinky_amd as bk
    pair = "local function pair(a, b) return a + b, a - b end\n"
    ok = LP.make_context(bk, pair + LP.lens("return x, y, z, x, pair(x, y)"), "four_and_call")
    assert ok.eval_host(1, 1.0, 2.0, 3.0) == (1.0, 2.0, 3.0, 1.0, 3.0, -1.0)
    ok.kernel_source()
    ok.close()
    for body, message in (("return x, y, z, x, y, pair(x, y)", "more than 4 return values in front of a trailing call"),
                          ("local a = x + y\nreturn x, y, z, x, y, z, x, y, a", "more than 8 return values")):
        ctx = LP.make_context(bk, pair + LP.lens(body), "too_many")
        with pytest.raises(bk.BlinkyError, match=message):
            ctx.kernel_source()
        ctx.close()
