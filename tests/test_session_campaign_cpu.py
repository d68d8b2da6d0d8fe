"""Random SESSIONS on one device-less context (tests/sessiongen.py): what bk_build keeps from one build to the next, as far as it can be
checked without a GPU.  After every step's transitions the host build paths (bk_debug_host_build, the mode drawn per step) must give the
table a FRESH oracle state gives for the model's globe / lens / zoom / size / grid, rows [r0, r1) of it, bit for bit; an error step must
answer with its error.  For a few seeds the GENERATED DEVICE CODE - bk_debug_kernel_source, which goes through the same remembered
translation unit (LensProgram::emitted) as bk_build and bk_build's asynchronous-compile gate - is compiled for the host and run
(tests/hostemu) at every step whose lens has an inverse map, by the rule of tests/test_exactness_cpu.py: every entry that differs from the
oracle's is in the flagged list.  Every step ends with kernel_source(), which leaves the remembered answer at the current activity count,
as a bk_build of a stateless lens leaves it (KeepActivity): the next step's transitions then meet the state they would meet on a GPU.
BLINKY_SESSION_CAMPAIGN=lo:hi runs a developer campaign."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostemu"))

import emu              # noqa: E402
import oracle_ffi as O  # noqa: E402
import scripts as S     # noqa: E402
import sessiongen as G  # noqa: E402

COMMITTED = range(24)                     # (G.GPU_COMMITTED, the GPU campaign's range, is the first 16 of them)
EMU_SEEDS = (2, 17, 19)                    # g++ compiles one object per distinct generated source: three sessions, about a dozen sources


def _seeds():
    v = os.environ.get("BLINKY_SESSION_CAMPAIGN")
    if not v:
        return COMMITTED
    lo, hi = [int(x) for x in v.split(":")]
    return range(lo, hi)


def run_session(seed, with_emu, request):
    import blinky_amd as bk
    request.addfinalizer(lambda: bk.debug_set_option("forward_careful", 0))      # (a process-wide option)
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    log = []
    inverse_steps = []                      # the steps whose map the device's inverse kernel builds: (index, at the globe_plate edge with no script run)
    for st in G.session(seed):
        e = st.expect
        for call in st.calls:
            log.append(call)
            if call[0] not in G.GPU_ONLY:
                try:
                    G.run_call(ctx, call)
                except Exception as err:      # (a transition that raises reports its own step and the calls so far)
                    raise AssertionError(f"{call} raised {type(err).__name__}: {err}\nseed {seed} step {st.index} {st.kinds}: {e}\ncalls so far: {log}") from err
        where = f"seed {seed} step {st.index} {st.kinds}: {e}\ncalls so far: {log}"
        assert ctx.size()[:2] == (e.W, e.H) and ctx.size()[3:] == e.rows, where
        if e.error:
            with pytest.raises(bk.ffi.BlinkyError, match=e.error):
                ctx.host_build(st.host_mode)
            continue
        W, H, (r0, r1) = e.W, e.H, e.rows
        lm = O.lensmap(e.globe, e.lens, e.zoom, W, H, e.grid)
        want_off = lm.offsets.reshape(H, W)[r0:r1].ravel()
        want_tin = lm.tints.reshape(H, W)[r0:r1].ravel()
        info = ctx.lens_info()
        if lm.built and info.has_inverse and info.map_type == bk.ffi.MAP_INVERSE:
            inverse_steps.append((st.index, G.EDGE in st.kinds and "load_lens" not in [c[0] for c in st.calls]))
        if with_emu and inverse_steps and inverse_steps[-1][0] == st.index:
            off, tin, flagged, err = emu.build_inverse(ctx)
            assert err == 0, where
            off = emu.device_to_reference_layout(off, min(W, H))
            differs = np.flatnonzero((off != want_off) | (tin != want_tin))
            missed = np.setdiff1d(differs, flagged)
            assert missed.size == 0, f"generated device code: {differs.size} of {off.size} entries differ from the oracle's, {missed.size} of them not flagged\n{where}"
        try:
            off, tin, display, scale, err = ctx.host_build(st.host_mode)
            built = err is None
        except bk.ffi.BlinkyError:
            built = False
        assert built == lm.built, where
        if built:
            bad = np.flatnonzero(off != want_off)
            assert bad.size == 0, f"host_build({st.host_mode}): {bad.size} of {off.size} offsets differ, first at {divmod(int(bad[0]), W)}\n{where}"
            assert np.array_equal(tin, want_tin), where
            assert scale == lm.scale or (scale != scale and lm.scale != lm.scale), where
            if (r0, r1) == (0, H):
                assert display[: lm.numplates] == lm.display, where
        try:
            ctx.kernel_source()            # (what a bk_build leaves behind: the translation unit remembered at the count of this moment)
        except bk.ffi.BlinkyError:
            pass
    ctx.close()
    return inverse_steps


@pytest.mark.parametrize("seed", _seeds())
def test_random_session_host_paths(seed, request):
    run_session(seed, False, request)


@pytest.mark.parametrize("seed", EMU_SEEDS)
def test_random_session_generated_device_code(seed, request):
    """... and each of these sessions leaves a globe script with a globe_plate function through bk_set_globe_plates, no script run in between,
    at a step whose device code is emulated: the edge at which a remembered translation unit was handed out again (r6)"""
    emulated = run_session(seed, True, request)
    assert len(emulated) >= 3 and any(edge for _, edge in emulated), emulated


def test_committed_sessions_hold_every_kind_of_transition():
    """the seed range the GPU campaign commits executes every kind of transition and every apply route at least once, the edge above in most
    sessions"""
    seeds = G.GPU_COMMITTED
    c, nsteps = G.census(seeds)
    missing = [k for k in G.KINDS if not c[k]] + [r for r in G.ROUTES if not c["route_" + r]]
    assert not missing, (missing, dict(c))
    with_edge = sum(any(G.EDGE in st.kinds for st in G.session(s)) for s in seeds)
    assert with_edge > len(seeds) // 2, with_edge
    assert all(10 <= len(G.session(s)) <= 14 for s in seeds)


def _emulated_table(ctx, W, H):
    off, tin, flagged, err = emu.build_inverse(ctx)
    assert err == 0
    return emu.device_to_reference_layout(off, min(W, H)), tin, flagged


@pytest.mark.parametrize("via_clear", [False, True])
def test_plates_set_after_a_globe_plate_script_regenerate_the_device_code(via_clear):
    """(r6 finding) `fast` (a globe_plate function) + panini, f_fov 200, 96 x 60; the device code is generated; then bk_set_globe_plates with the
    cube's plates, no script run in between.  The translation unit remembered for `fast` (BK_HAS_GLOBE_PLATE) must not be handed out again:
    the generated code, run on the host, is the oracle's cube / panini table up to its flagged entries (3232 of 5760 entries differed, none
    flagged), as the host path's table on the same context is."""
    import blinky_amd as bk
    W, H, zoom = 96, 60, "f_fov 200"
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    S.configure(ctx, "fast", "panini", zoom, (W, H))
    assert "BK_HAS_GLOBE_PLATE" in ctx.kernel_source()
    lm = O.lensmap("fast", "panini", zoom, W, H)
    off, tin, flagged = _emulated_table(ctx, W, H)
    assert set(np.flatnonzero((off != lm.offsets) | (tin != lm.tints)).tolist()) <= set(flagged.tolist())
    ctx.kernel_source()
    if via_clear:
        ctx.clear_globe()
        with pytest.raises(bk.ffi.BlinkyError, match="not a valid globe"):
            ctx.host_build(1)
    ctx.set_globe_plates(G.named_plates("cube"))
    assert "BK_HAS_GLOBE_PLATE" not in ctx.kernel_source()
    lm = O.lensmap("cube", "panini", zoom, W, H)
    off, tin, flagged = _emulated_table(ctx, W, H)
    differs = np.flatnonzero((off != lm.offsets) | (tin != lm.tints))
    assert set(differs.tolist()) <= set(flagged.tolist()), f"{differs.size} of {off.size} entries differ from the oracle's cube / panini table, {len(flagged)} flagged"
    hoff, htin, display, scale, err = ctx.host_build(1)
    assert err is None and scale == lm.scale and display[: lm.numplates] == lm.display
    np.testing.assert_array_equal(hoff, lm.offsets)
    np.testing.assert_array_equal(htin, lm.tints)
    ctx.close()


def test_set_globe_plates_leaves_numplates_to_the_next_lens_load():
    """What bk_set_globe_plates promises (include/blinky_hip.h): it runs no script and leaves the script state alone - the global `numplates` is
    bk_load_lens'.  lenses/debug.lua lays out its grid from numplates while its chunk runs: under the cube it is 3 cells wide; with the
    tetrahedron's four plates set it stays 3 wide until it is loaded again, as the reference loads the lens again after every f_globe, and is
    then 2 wide and builds the oracle's tetra / debug table."""
    import blinky_amd as bk
    W, H = 64, 48
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    S.configure(ctx, "cube", "debug", None, (W, H))
    assert ctx.lens_info().lens_width == 3
    ctx.set_globe_plates(G.named_plates("tetra"))
    assert len(ctx.globe()) == 4 and ctx.lens_info().lens_width == 3
    ctx.load_lens(S.script("lenses", "debug"), "debug.lua")
    assert ctx.lens_info().lens_width == 2
    lm = O.lensmap("tetra", "debug", None, W, H)
    off, tin, display, scale, err = ctx.host_build(0)
    assert err is None and scale == lm.scale
    np.testing.assert_array_equal(off, lm.offsets)
    np.testing.assert_array_equal(tin, lm.tints)
    ctx.close()


def test_clear_lens_and_clear_globe_are_bound():
    """ffi.Context.clear_lens / clear_globe: the build answers "not a valid lens / globe" until a good load"""
    import blinky_amd as bk
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    S.configure(ctx, "cube", "panini", None, (32, 24))
    assert ctx.host_build(1)[4] is None
    ctx.clear_lens()
    with pytest.raises(bk.ffi.BlinkyError, match="not a valid lens"):
        ctx.host_build(1)
    ctx.load_lens(S.script("lenses", "panini"), "panini.lua")
    ctx.clear_globe()
    assert ctx.globe() == []
    with pytest.raises(bk.ffi.BlinkyError, match="not a valid globe"):
        ctx.host_build(1)
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    assert ctx.host_build(1)[4] is None
    ctx.close()


def test_only_the_listed_lenses_read_numplates():
    """the generator loads a lens again after bk_set_globe_plates only where its chunk depends on the globe (G.NUMPLATES_LENSES): no other
    shipped lens names the global numplates, or the `plates` table a globe script leaves behind"""
    import re
    readers = [l for l in S.LENSES if re.search(r"\b(numplates|plates)\b", S.script("lenses", l))]
    assert tuple(readers) == G.NUMPLATES_LENSES


def test_a_deviceless_resize_to_the_size_it_has_keeps_the_stripe():
    """bk_resize to the current size is a no-op on a device-less context as it is with a device: the rows set by bk_set_rows stay; another
    size lifts them"""
    import blinky_amd as bk
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    ctx.resize(40, 30)
    ctx.set_rows(7, 19)
    ctx.resize(40, 30)
    assert ctx.size() == (40, 30, 30, 7, 19)
    ctx.resize(30, 40)
    assert ctx.size() == (30, 40, 30, 0, 40)
    ctx.close()
