"""Random SESSIONS on one Context (tests/sessiongen.py): what bk_build and the apply keep from one build to the next - the generated
translation unit, the forward build's tables and scratch, the two compiled block maps, the resident kernel with a block map in its
registers - put through what nobody picked: scripts, plates and sizes changing under a context that has built before, builds that fail and
the good load after them, a resident session that stays open while the table under it is rebuilt.  After EVERY step's build the table, the
zoom scale, the display flags and `built` are the oracle's for the model's configuration, rows [r0, r1) of it; then the step's frames -
bk_apply_device, the host bk_apply, a resident session, the drop-in mode - are the oracle's apply over the oracle's table, byte for byte,
on a frame prefilled with a sentinel.  A build that fails leaves the lensmap valid and empty: the frame stays as it was.
The committed range runs in seconds; BLINKY_SESSION_CAMPAIGN=lo:hi runs a developer campaign.  Bit-exact."""
import os
import time

import numpy as np
import pytest

import oracle_ffi as O
import scripts as S
import sessiongen as G

pytestmark = pytest.mark.gpu

SENTINEL = 77


def _seeds():
    v = os.environ.get("BLINKY_SESSION_CAMPAIGN")
    if not v:
        return G.GPU_COMMITTED
    lo, hi = [int(x) for x in v.split(":")]
    return range(lo, hi)


class _Where:
    """seed, step and the calls made so far, formatted when a failure message needs it"""

    def __init__(self, head, log):
        self.head, self.log = head, log

    def __str__(self):
        return f"{self.head}\ncalls so far: {self.log}"


class Session:
    def __init__(self, bk, seed):
        self.bk, self.seed = bk, seed
        self.ctx = bk.Context()
        self.log = []
        self.globes = {}                      # ring slot -> the plates it holds
        self.dirty = True                     # the ring was (re)allocated: its plates are gone
        self.epoch = 0
        self.nframes = 1
        self.pal = O.palmap(((np.arange(768) * (17 + 2 * seed) + 11) % 256).astype(np.uint8))
        self.held = None                      # a resident session / the drop-in mode left open by the last step: (kind, rubix, frames to compare at its end)
        self.where = ""

    # ---- the calls only a device context takes
    def flush_plates(self):
        if not self.dirty:
            return
        ps = self.ctx.size()[2]
        self.epoch += 1
        for f in range(self.nframes):
            self.globes[f] = O.lcg_globe(ps, 6, 1000 * self.seed + 16 * self.epoch + f)
            for p in range(6):
                self.ctx.upload_plate(f, p, self.globes[f][p])
        self.dirty = False

    def call(self, call):
        self.log.append(call)
        if call[0] == "set_frames":
            self.ctx.set_frames(call[1])
            self.nframes = call[1]
            self.dirty = True
        elif call[0] == "set_lensmap":
            self.arbitrary_table(call[1])
        else:
            before = self.ctx.size()[:2]
            G.run_call(self.ctx, call)
            if call[0] == "resize" and self.ctx.size()[:2] != before:
                self.dirty = True

    def arbitrary_table(self, tseed):
        """bk_set_lensmap with a table no lens produces and one launch over it (a block map is compiled for it): the build that follows must
        leave nothing of either"""
        import torch
        W, H, ps, r0, r1 = self.ctx.size()
        rng = np.random.default_rng(tseed)
        off = rng.integers(0, 6 * ps * ps, W * H, dtype=np.uint32)
        off[rng.random(W * H) < 0.1] = O.NULL
        tin = rng.integers(0, 6, W * H).astype(np.uint8)
        self.ctx.set_lensmap(off.reshape(H, W)[r0:r1].ravel(), tin.reshape(H, W)[r0:r1].ravel())
        self.flush_plates()
        route = dict(pitch=W, x0=0, y0=0)
        out = torch.full((H + 2, W), SENTINEL, dtype=torch.uint8, device="cuda")
        self.ctx.apply_device(out.data_ptr(), W, (H + 2) * W, frame0=0, nframes=1)
        self.ctx.synchronize()
        torch.cuda.synchronize()
        self.compare(out.cpu().numpy(), self.want(off, tin, route, 0, False), "bk_set_lensmap's table")

    # ---- expectations
    def want(self, off, tin, route, slot, rubix):
        W, H, ps, r0, r1 = self.ctx.size()
        pitch, x0, y0 = route["pitch"], route["x0"], route["y0"]
        FH = H + y0 + 2
        full = np.full((FH, pitch), SENTINEL, np.uint8)
        O.apply(off, tin, W, H, self.globes[slot], full, pitch, x0, y0, rubix, self.pal if rubix else None)
        want = np.full((FH, pitch), SENTINEL, np.uint8)
        want[y0 + r0:y0 + r1] = full[y0 + r0:y0 + r1]            # a stripe context writes its rows only
        return want

    def compare(self, got, want, what):
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{what}: {len(bad)} bytes differ, first at (y, x) = {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}\n{self.where}")

    # ---- one step
    def step(self, st, last):
        import torch
        bk, ctx, e = self.bk, self.ctx, st.expect
        # (set before the calls run - a transition that raises reports this step - and `log` grows in place as they do)
        self.where = _Where(f"seed {self.seed} step {st.index} {st.kinds} route {st.route}: {e}", self.log)
        for call in st.calls:
            try:
                self.call(call)
            except AssertionError:
                raise
            except Exception as err:
                raise AssertionError(f"{call} raised {type(err).__name__}: {err}\n{self.where}") from err
        W, H, ps, r0, r1 = ctx.size()
        assert (W, H, r0, r1) == (e.W, e.H) + e.rows, str(self.where)
        self.flush_plates()
        # build and check
        lm = None if e.error else O.lensmap(e.globe, e.lens, e.zoom, W, H, e.grid)
        try:
            display, scale = ctx.build()
            built = True
        except bk.ffi.BlinkyError as err:
            built = False
            if e.error:
                assert e.error in str(err), f"{err}\n{self.where}"
        assert built == (lm is not None and lm.built), str(self.where)
        off, tin = ctx.read_lensmap()
        if built:
            want_off = lm.offsets.reshape(H, W)[r0:r1].ravel()
            bad = np.flatnonzero(off != want_off)
            assert bad.size == 0, (f"{bad.size} of {off.size} offsets differ, first at (y, x) = {divmod(int(bad[0]), W)} (stripe row): {off[bad[0]]} != "
                                   f"{want_off[bad[0]]}; fixups {ctx.last_build_fixups()}\n{self.where}")
            assert np.array_equal(tin, lm.tints.reshape(H, W)[r0:r1].ravel()), str(self.where)
            assert scale == lm.scale or (scale != scale and lm.scale != lm.scale), f"scale {scale!r} != {lm.scale!r}\n{self.where}"
            if (r0, r1) == (0, H):
                assert display[: lm.numplates] == lm.display, str(self.where)
            else:                                                # a stripe sees the plates its own rows read (forward maps: all of them)
                assert all(d <= w for d, w in zip(display[: lm.numplates], lm.display)), str(self.where)
            # the shipped lenses carry no state and the emitter takes them all: the host scan only where it was asked for
            assert ctx.last_build_path()[0] == (2 if e.seq == 2 else 0), f"{ctx.last_build_path()}\n{self.where}"
            t_off, t_tin = lm.offsets, lm.tints
        else:
            # "whatever fails, the lensmap stays valid-and-empty so that bk_apply draws nothing" (bk_build)
            assert (off == O.NULL).all() and (tin == 255).all(), str(self.where)
            t_off, t_tin = np.full(W * H, O.NULL, np.uint32), np.full(W * H, 255, np.uint8)
        # apply and check
        r = st.route
        kind, pitch, x0, y0, rubix = r["kind"], r["pitch"], r["x0"], r["y0"], r["rubix"]
        FH = H + y0 + 2
        slot = r["frame0"] % self.nframes
        pal = self.pal
        if kind.startswith("continue_"):
            hkind, hrubix, pending = self.held
            self.held = None
            if hkind == "resident_hold":
                out = torch.full((FH, pitch), SENTINEL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()                         # (bk_build has taken the kernel off the device; the session is still open)
                ctx.resident_wait(ctx.resident_submit(out.data_ptr(), pitch, frame=slot, x0=x0, y0=y0))
                info = ctx.resident_info()
                ctx.resident_end()
                torch.cuda.synchronize()
                pending.append((out, self.want(t_off, t_tin, r, slot, hrubix), f"the session's frame after the rebuild ({info})"))
            else:
                frame = np.full((FH, pitch), SENTINEL, np.uint8)
                ctx.apply(frame, slot, pitch, x0, y0, hrubix, pal if hrubix else None)
                ctx.set_resident_apply(False)
                pending.append((frame, self.want(t_off, t_tin, r, slot, hrubix), "the drop-in mode's frame after the rebuild"))
            for got, want, what in pending:
                self.compare(got if isinstance(got, np.ndarray) else got.cpu().numpy(), want, what)
        elif kind in ("device", "device_flip"):
            nf = r["nf"]
            for rep in range(3 if kind == "device_flip" else 2):   # (the second launch runs on the block map the first one compiled; a flip changes its flavour)
                rbx = (not rubix) if (kind == "device_flip" and rep == 1) else rubix
                out = torch.full((nf, FH, pitch), SENTINEL, dtype=torch.uint8, device="cuda")
                ctx.apply_device(out.data_ptr(), pitch, FH * pitch, frame0=slot, nframes=nf, x0=x0, y0=y0, rubix_on=rbx, pal=pal)
                ctx.synchronize()
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                for f in range(nf):
                    self.compare(got[f], self.want(t_off, t_tin, r, (slot + f) % self.nframes, rbx), f"launch {rep} frame {f} rubix {rbx}")
        elif kind == "host":
            frame = np.full((FH, pitch), SENTINEL, np.uint8)
            ctx.apply(frame, slot, pitch, x0, y0, rubix, pal if rubix else None)
            self.compare(frame, self.want(t_off, t_tin, r, slot, rubix), "bk_apply")
        elif kind == "resident_hold":
            out = torch.full((FH, pitch), SENTINEL, dtype=torch.uint8, device="cuda")
            ctx.synchronize()
            torch.cuda.synchronize()
            ctx.resident_begin(rubix, pal if rubix else None, idle_ms=2000)
            ctx.resident_wait(ctx.resident_submit(out.data_ptr(), pitch, frame=slot, x0=x0, y0=y0))
            pending = [(out, self.want(t_off, t_tin, r, slot, rubix), "the session's frame before the rebuild")]
            if last:
                ctx.resident_end()
                torch.cuda.synchronize()
                self.compare(out.cpu().numpy(), pending[0][1], pending[0][2])
            else:
                self.held = (kind, rubix, pending)               # (read once the session has ended: nothing else touches the device while its kernel runs)
        else:
            assert kind == "resident_mode", kind
            ctx.set_resident_apply(True)
            frame = np.full((FH, pitch), SENTINEL, np.uint8)
            ctx.apply(frame, slot, pitch, x0, y0, rubix, pal if rubix else None)
            self.compare(frame, self.want(t_off, t_tin, r, slot, rubix), "bk_apply in drop-in mode")
            if last:
                ctx.set_resident_apply(False)
            else:
                self.held = (kind, rubix, [])


@pytest.mark.parametrize("seed", _seeds())
def test_random_session(seed, request):
    import blinky_amd as bk
    request.addfinalizer(lambda: bk.debug_set_option("forward_careful", 0))      # (a process-wide option)
    t0 = time.perf_counter()
    s = Session(bk, seed)
    steps = G.session(seed)
    for st in steps:
        s.step(st, st is steps[-1])
    s.ctx.close()
    ntrans = sum(k not in ("initial", G.EDGE) for st in steps for k in st.kinds)
    print(f"session {seed}: {len(steps)} steps, {ntrans} transitions, {time.perf_counter() - t0:.2f} s")


# ---- the edge the campaign was written for, directed ------------------------------------------------------------------------------------

def _fast_panini(bk, W, H, zoom):
    ctx = bk.Context()
    S.configure(ctx, "fast", "panini", zoom, (W, H))
    display, scale = ctx.build()
    lm = O.lensmap("fast", "panini", zoom, W, H)
    off, tin = ctx.read_lensmap()
    assert np.array_equal(off, lm.offsets) and np.array_equal(tin, lm.tints) and display[: lm.numplates] == lm.display
    return ctx


def _is_cube_panini(ctx, result, W, H, zoom):
    display, scale = result
    lm = O.lensmap("cube", "panini", zoom, W, H)
    off, tin = ctx.read_lensmap()
    bad = np.flatnonzero(off != lm.offsets)
    assert bad.size == 0, f"{bad.size} of {off.size} offsets differ from the oracle's cube / panini table, first at (y, x) = {divmod(int(bad[0]), W)}"
    np.testing.assert_array_equal(tin, lm.tints)
    assert display[: lm.numplates] == lm.display and scale == lm.scale


@pytest.mark.parametrize("via_clear", [False, True])
def test_plates_set_after_a_globe_plate_script_rebuild_for_the_plates(via_clear):
    """(r6 finding) `fast` - a globe script with a globe_plate function - + panini, f_fov 200, 320 x 200, built; then bk_set_globe_plates with
    the cube's plates (or bk_clear_globe first), no script run in between: the next build must not reuse the translation unit generated for
    `fast` (BK_HAS_GLOBE_PLATE) - table, display flags and scale are the oracle's for cube / panini"""
    import blinky_amd as bk
    W, H, zoom = 320, 200, "f_fov 200"
    ctx = _fast_panini(bk, W, H, zoom)
    if via_clear:
        ctx.clear_globe()
    ctx.set_globe_plates(G.named_plates("cube"))
    _is_cube_panini(ctx, ctx.build(), W, H, zoom)
    assert ctx.last_build_path()[0] == 0
    ctx.close()


def test_plates_set_after_a_globe_plate_script_with_asynchronous_compilation():
    """... and under bk_set_async_compile, whose gate (build_module_ready) consults the same remembered translation unit"""
    import blinky_amd as bk
    W, H, zoom = 320, 200, "f_fov 200"
    ctx = _fast_panini(bk, W, H, zoom)
    ctx.set_async_compile(True)
    ctx.set_globe_plates(G.named_plates("cube"))
    deadline = time.time() + 120
    while (res := ctx.build_nowait()) is None:
        assert time.time() < deadline
        time.sleep(0.01)
    _is_cube_panini(ctx, res, W, H, zoom)
    ctx.close()
