"""TEST INFRASTRUCTURE: random SESSIONS for the campaigns that keep one context through many rebuilds
(tests/test_session_campaign_cpu.py, tests/test_session_campaign_gpu.py).

The other campaigns treat a seed as one configuration on a fresh Context.  bk_build keeps things from one build to the next - the
generated translation unit (LensProgram::emitted, keyed on the interpreter's activity count and rewound by KeepActivity), the forward
build's tables and scratch, the two compiled block maps, the resident kernel - and decides per build which of them still hold.  Here a
seed is a whole session: one context, 10-14 steps, each step a few TRANSITIONS followed by "build and check".  The generator keeps a
model of what the context was told - globe, lens, zoom command, size, rows, grid - and that model is all the oracle is asked for:
O.lensmap(globe, lens, zoom, W, H, grid) of a FRESH state is the expectation for a long-lived context, rows [r0, r1) of it.

A step is data: `calls` (tuples, run by `run_call`; the GPU-only ones are skipped on a device-less context), `kinds` (the names the
coverage census counts), the model after the transitions (`expect`), how the frame is applied on a GPU (`route`) and which host path the
CPU campaign takes (`host_mode`).  Both campaigns draw from the same stream, so a seed names the same session in either."""
import collections

import numpy as np

import scripts as S

BASE_SEED = 31000
GPU_COMMITTED = range(16)        # the seeds tests/test_session_campaign_gpu.py runs in the suite; the census test holds this range to every kind

# every kind of transition a step can hold; the census test wants each of them in the committed seed range
KINDS = (
    # scripts
    "load_lens_other", "load_lens_same", "load_globe", "set_globe_plates", "set_globe_plates_reload", "clear_globe_set_plates",
    "clear_lens_load_lens",
    # geometry
    "resize_new", "resize_transposed", "resize_same", "rows_stripe", "rows_shift", "rows_full", "rubixgrid",
    "zoom_fov", "zoom_vfov", "zoom_cover", "zoom_contain", "zoom_onload", "frames_grow", "frames_shrink",
    # build path
    "sequential_0", "sequential_1", "sequential_2", "same_build_twice", "calc_zoom", "eval_host", "forward_careful", "set_lensmap",
    # errors that are answers
    "bad_lens_chunk", "clear_lens_build", "clear_globe_build", "recover",
)
ROUTES = ("device", "device_flip", "host", "resident_hold", "resident_mode")
# the one edge the campaigns were written for: a globe SCRIPT with a globe_plate function, then plates set without any script running
EDGE = "globe_plate_to_plates"

# chunks that fail to load: a call to error(), a run-time error AFTER the chunk has defined a callback (the global stays behind in the
# script state, the lens is invalid all the same), a syntax error
BAD_LENSES = (
    "lens_width = 2\nerror('no such projection')\n",
    "function lens_inverse(x, y) return 0, 0, 1 end\nmax_fov = 100\nlocal t = nil\nt.x = 1\n",
    "max_fov = = 3\n",
)
# set_globe_plates hands over a named globe's plates WITHOUT its globe_plate function: for `fast`, whose script picks plates with one, that is
# a globe no script describes (and the oracle has no name for)
PLATE_GLOBES = tuple(g for g in S.GLOBES if g != "fast")
# the one shipped lens whose CHUNK reads the script global numplates (lenses/debug.lua:1-14 lays its grid out from it): bk_set_globe_plates
# leaves script state alone (include/blinky_hip.h), so after it this lens is always loaded again, as the reference does after f_globe
# (established by searching the shipped scripts for `numplates`: lenses/debug.lua is the only file of tests/golden/scripts.bundle that names it,
# and no lens reads `plates` or another global a globe script sets; test_only_the_listed_lenses_read_numplates repeats the search)
NUMPLATES_LENSES = ("debug",)

Step = collections.namedtuple("Step", "index calls kinds expect route host_mode")
Expect = collections.namedtuple("Expect", "globe lens zoom W H grid rows error seq nframes")


def _zoom(rng):
    deg = int(rng.choice([10, 45, 60, 90, 100, 120, 150, 179, 180, 181, 200, 270, 359, 360])) if rng.random() < 0.6 else int(rng.integers(1, 400))
    kind = str(rng.choice(["zoom_fov", "zoom_vfov", "zoom_cover", "zoom_contain", "zoom_onload"]))
    return kind, {"zoom_fov": f"f_fov {deg}", "zoom_vfov": f"f_vfov {deg}", "zoom_cover": "f_cover", "zoom_contain": "f_contain", "zoom_onload": None}[kind]


def _stripe(rng, H):
    r0 = int(rng.integers(0, H - 1))
    return r0, int(rng.integers(r0 + 1, H + 1))


def _route(rng, W, nframes, held):
    """how a step's frame is applied on a GPU.  resident_hold / resident_mode leave their session open across the NEXT step's transitions and
    build; that step's route is the rest of it (continue_...): the same session against the new table, then its end"""
    kind = str(rng.choice(ROUTES, p=[0.3, 0.15, 0.15, 0.25, 0.15]))
    if held:
        kind = "continue_" + held
    pitch = W + int(rng.integers(0, 9))
    return dict(kind=kind, pitch=pitch, x0=int(rng.integers(0, pitch - W + 1)), y0=int(rng.integers(0, 4)), rubix=bool(rng.random() < 0.45),
                frame0=int(rng.integers(0, nframes)), nf=int(rng.integers(1, 4)))


def session(seed):
    """-> list of Step for this seed"""
    rng = np.random.default_rng(BASE_SEED + seed)
    pool = [str(x) for x in rng.choice(S.LENSES, 3, replace=False)]
    nsteps = int(rng.integers(10, 15))
    m = dict(globe=None, globe_script=False, lens=pool[0], zoom=None, W=0, H=0, grid=(10, 4.0, 1.0), rows=(0, 0), error=None, seq=0,
             nframes=int(rng.integers(1, 4)), careful=0)
    steps = []

    def load_globe(calls, name):
        calls.append(("load_globe", name))
        m["globe"], m["globe_script"] = name, True

    def load_lens(calls, name):
        calls.append(("load_lens", name))
        calls.append(("zoom", m["zoom"]))                  # (cmd_lens runs the lens' onload; a zoom command given since then is given again)
        m["lens"] = name

    def set_plates(calls, kinds, name, kind):
        if m["globe_script"] and m["globe"] == "fast":
            kinds.append(EDGE)
        calls.append(("set_globe_plates", name))
        m["globe"], m["globe_script"] = name, False
        reload_ = m["lens"] in NUMPLATES_LENSES or rng.random() < 0.3
        if reload_:
            load_lens(calls, m["lens"])
        kinds.append(kind + "_reload" if reload_ and kind == "set_globe_plates" else kind)

    def other_plates():
        return str(rng.choice([g for g in PLATE_GLOBES if g != m["globe"]]))

    for k in range(nsteps):
        calls, kinds = [], []
        if k == 0:
            calls.append(("set_frames", m["nframes"]))
            load_globe(calls, "fast" if rng.random() < 0.5 else str(rng.choice(S.GLOBES)))
            m["zoom"] = _zoom(rng)[1]
            load_lens(calls, pool[0])
            m["W"], m["H"] = int(rng.integers(8, 201)), int(rng.integers(8, 151))
            m["rows"] = (0, m["H"])
            calls.append(("resize", m["W"], m["H"]))
            kinds.append("initial")
        elif m["error"]:
            # the step after an error recovers with a good load and must match the oracle again
            if m["error"] == "not a valid lens":
                load_lens(calls, str(rng.choice(pool)))
                kinds.append("recover")
            elif rng.random() < 0.5:
                set_plates(calls, kinds, other_plates(), "recover")
            else:
                load_globe(calls, str(rng.choice(S.GLOBES)))
                load_lens(calls, m["lens"])
                kinds.append("recover")
            m["error"] = None
        else:
            u = rng.random()
            if u < 0.07:
                kinds.append("same_build_twice")
            elif u < 0.19:
                which = str(rng.choice(["bad_lens_chunk", "clear_lens_build", "clear_globe_build"]))
                if which == "bad_lens_chunk":
                    calls.append(("load_bad_lens", int(rng.integers(0, len(BAD_LENSES)))))
                    m["error"] = "not a valid lens"
                elif which == "clear_lens_build":
                    calls.append(("clear_lens",))
                    m["error"] = "not a valid lens"
                else:
                    calls.append(("clear_globe",))
                    m["error"] = "not a valid globe"
                    m["globe"], m["globe_script"] = None, False
                kinds.append(which)
            else:
                for _ in range(int(rng.integers(1, 4))):
                    # `fast` under a globe script is the state the stale-source edge starts from: leave it through set_globe_plates more often than not
                    on_fast = m["globe_script"] and m["globe"] == "fast"
                    group = str(rng.choice(["scripts", "geometry", "path"], p=[0.6, 0.25, 0.15] if on_fast else [0.34, 0.4, 0.26]))
                    if group == "scripts":
                        t = str(rng.choice(["load_lens_other", "load_lens_same", "load_globe", "set_globe_plates", "clear_globe_set_plates", "clear_lens_load_lens"],
                                           p=[0.1, 0.06, 0.2, 0.42, 0.14, 0.08] if on_fast else [0.2, 0.1, 0.3, 0.2, 0.1, 0.1]))
                        if t == "load_lens_other":
                            load_lens(calls, str(rng.choice([x for x in pool if x != m["lens"]])))
                        elif t == "load_lens_same":
                            load_lens(calls, m["lens"])
                        elif t == "load_globe":
                            load_globe(calls, "fast" if rng.random() < 0.45 else str(rng.choice(S.GLOBES)))
                            load_lens(calls, m["lens"])            # (f_globe: the lens is loaded again, fisheye.c:730-741)
                        elif t == "set_globe_plates":
                            set_plates(calls, kinds, other_plates(), t)
                            continue
                        elif t == "clear_globe_set_plates":
                            name = other_plates()
                            calls.append(("clear_globe",))
                            set_plates(calls, kinds, name, t)
                            continue
                        else:
                            calls.append(("clear_lens",))
                            load_lens(calls, m["lens"])
                        kinds.append(t)
                    elif group == "geometry":
                        t = str(rng.choice(["resize_new", "resize_transposed", "resize_same", "rows", "rubixgrid", "zoom", "frames"],
                                           p=[0.14, 0.08, 0.06, 0.26, 0.1, 0.26, 0.1]))
                        if t == "rows":                                    # a stripe; from a stripe mostly the same row count somewhere else, or the whole frame again
                            full = m["rows"][1] - m["rows"][0] == m["H"]
                            t = "rows_stripe" if full else str(rng.choice(["rows_shift", "rows_full", "rows_stripe"], p=[0.5, 0.3, 0.2]))
                        if t.startswith("resize"):
                            if t == "resize_new":
                                m["W"], m["H"] = int(rng.integers(8, 201)), int(rng.integers(8, 151))
                            elif t == "resize_transposed":                 # the same pixel count: the tables' allocation is kept while W changes
                                m["W"], m["H"] = m["H"], m["W"]
                            calls.append(("resize", m["W"], m["H"]))
                            if t != "resize_same" and not (t == "resize_transposed" and m["W"] == m["H"]):
                                m["rows"] = (0, m["H"])                    # (bk_resize to another size lifts the stripe; the size it has is a no-op)
                        elif t == "rows_stripe":
                            m["rows"] = _stripe(rng, m["H"])
                            calls.append(("set_rows",) + m["rows"])
                        elif t == "rows_shift":                            # the same row count somewhere else: the tables' allocation is kept
                            n = m["rows"][1] - m["rows"][0]
                            r0 = int(rng.choice([r for r in range(0, m["H"] - n + 1) if r != m["rows"][0]]))
                            m["rows"] = (r0, r0 + n)
                            calls.append(("set_rows",) + m["rows"])
                        elif t == "rows_full":
                            m["rows"] = (0, m["H"])
                            calls.append(("set_rows",) + m["rows"])
                        elif t == "rubixgrid":
                            m["grid"] = (int(rng.integers(1, 24)), float(rng.choice([0.5, 1, 2, 4, 7.5])), float(rng.choice([0, 0.25, 1, 3])))
                            calls.append(("set_rubixgrid",) + m["grid"])
                        elif t == "zoom":
                            t, m["zoom"] = _zoom(rng)
                            calls.append(("zoom", m["zoom"]))
                        else:
                            grow = m["nframes"] == 1 or rng.random() < 0.5
                            m["nframes"] = m["nframes"] + int(rng.integers(1, 3)) if grow else int(rng.integers(1, m["nframes"]))
                            t = "frames_grow" if grow else "frames_shrink"
                            calls.append(("set_frames", m["nframes"]))
                        kinds.append(t)
                    else:
                        t = str(rng.choice(["sequential", "calc_zoom", "eval_host", "forward_careful", "set_lensmap"], p=[0.34, 0.16, 0.16, 0.16, 0.18]))
                        if t == "sequential":
                            m["seq"] = int(rng.choice([x for x in (0, 1, 2) if x != m["seq"]]))
                            t = "sequential_%d" % m["seq"]
                            calls.append(("set_sequential_build", m["seq"]))
                        elif t == "calc_zoom":
                            calls.append(("calc_zoom",))
                        elif t == "eval_host":
                            calls.append(("eval_host", float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.4, 0.4))))
                        elif t == "forward_careful":
                            m["careful"] ^= 1
                            calls.append(("forward_careful", m["careful"]))
                        else:
                            calls.append(("set_lensmap", int(rng.integers(0, 1 << 30))))
                        kinds.append(t)
        expect = Expect(m["globe"], m["lens"], m["zoom"], m["W"], m["H"], m["grid"], m["rows"], m["error"], m["seq"], m["nframes"])
        held = steps[-1].route["kind"] if steps and steps[-1].route["kind"] in ("resident_hold", "resident_mode") else None
        steps.append(Step(k, calls, kinds, expect, _route(rng, m["W"], m["nframes"], held), int(rng.integers(0, 3))))
    return steps


def census(seeds):
    """how often each kind of transition and each apply route occurs in the sessions of `seeds`: (Counter, number of steps)"""
    c = collections.Counter()
    n = 0
    for seed in seeds:
        for st in session(seed):
            n += 1
            c.update(st.kinds)
            c["route_" + st.route["kind"]] += 1
    return c, n


_plates = {}


def named_plates(name):
    """the plates of a shipped globe in bk_set_globe_plates' form, from a scratch device-less context"""
    if name not in _plates:
        import blinky_amd as bk
        c = bk.Context(bk.ffi.DEVICE_NONE)
        c.load_globe(S.script("globes", name), name + ".lua")
        _plates[name] = c.globe()
        c.close()
    return _plates[name]


GPU_ONLY = ("set_frames", "set_lensmap")


def run_call(ctx, call):
    """one call of a step on a blinky_amd Context (the GPU campaign handles GPU_ONLY itself)"""
    import blinky_amd as bk
    op, args = call[0], call[1:]
    if op == "load_globe":
        ctx.load_globe(S.script("globes", args[0]), args[0] + ".lua")
    elif op == "load_lens":
        ctx.load_lens(S.script("lenses", args[0]), args[0] + ".lua")
    elif op == "load_bad_lens":
        try:
            ctx.load_lens(BAD_LENSES[args[0]], "bad.lua")
        except bk.ffi.BlinkyError as e:
            assert "could not load lens" in str(e), str(e)
        else:
            raise AssertionError("a lens chunk that fails was loaded without an error")
    elif op == "set_globe_plates":
        ctx.set_globe_plates(named_plates(args[0]))
    elif op == "clear_globe":
        ctx.clear_globe()
    elif op == "clear_lens":
        ctx.clear_lens()
    elif op == "zoom":
        ctx.set_zoom(*S.zoom_args(args[0] if args[0] else ctx.lens_info().onload.decode()))
    elif op == "resize":
        ctx.resize(*args)
    elif op == "set_rows":
        ctx.set_rows(*args)
    elif op == "set_rubixgrid":
        ctx.set_rubixgrid(*args)
    elif op == "set_sequential_build":
        ctx.set_sequential_build(args[0])
    elif op == "calc_zoom":
        try:
            ctx.calc_zoom()
        except bk.ffi.BlinkyError:
            pass                                         # (a zoom the lens cannot give: the build says the same, and the oracle says `not built`)
    elif op == "eval_host":
        info = ctx.lens_info()
        try:
            ctx.eval_host(0, *args) if info.has_inverse else ctx.eval_host(1, args[0], args[1], 1.0)
        except bk.ffi.BlinkyError:
            pass
    elif op == "forward_careful":
        bk.debug_set_option("forward_careful", args[0])
    else:
        raise ValueError(call)
