// bk_lens.cpp -- the script side of the C ABI: globe / lens loading, zoom, and the lens module (emit -> code object -> loaded
// kernels); the builds that launch them are bk_build.cpp.  Host logic mirrors fisheye.c's LUA_load_globe (1752-1875),
// LUA_load_lens (1659-1750) and calc_zoom (1293-1386).
#include <chrono>
#include <cstring>
#include <future>

#include "bk_emit.h"
#include "bk_lens_priv.h"

using namespace bklua;

namespace bk {

static double need_num(const Values &a, size_t i, const char *fn)
{
    if (i >= a.size() || a[i].t != Value::NUM)
        throw LuaError(std::string("bad argument #") + std::to_string(i + 1) + " to '" + fn + "' (number expected)");
    return a[i].n;
}

// Host-side script execution (chunks, calc_zoom, globe loading) runs on the PLATFORM libm by
// default: that is what the reference's Lua VM calls on this machine, so lens.scale, lens_width,
// plate vectors etc. come out bit-identical to the reference's.  bk_set_host_math() switches
// to the portable bkm.h functions (= what the GPU kernels use) for platform-independent results.
LensProgram::LensProgram(bk_ctx *ctx) : interp(math_platform())
{
    interp.print_sink = [this](const std::string &s) { console += s; };          // (print's lines with their newline, io.write's text as it is)
    // the aliases init_lua installs (fisheye.c:1230-1248): cos = math.cos ... tau = math.pi*2
    static const char *alias[] = {"cos", "sin", "tan", "asin", "acos", "atan", "atan2", "sinh", "cosh", "tanh",
                                  "log", "log10", "abs", "sqrt", "exp", "pow"};
    Value math = interp.get_global("math");
    for (const char *a : alias) interp.set_global(a, math.tab()->get(Value::string(a)));
    interp.set_global("pi", math.tab()->get(Value::string("pi")));
    interp.set_global("tau", Value::number(math.tab()->get(Value::string("pi")).n * 2));
    // the three C functions scripts may call (fisheye.c:1257-1264, 1494-1537)
    interp.register_builtin("latlon_to_ray", [](Interp &I, const Values &a, Values &r) {
        float ray[3];
        h_latlon_to_ray(*I.math, need_num(a, 0, "latlon_to_ray"), need_num(a, 1, "latlon_to_ray"), ray);
        for (int i = 0; i < 3; ++i) r.push_back(Value::number((double)ray[i]));
    });
    interp.register_builtin("ray_to_latlon", [](Interp &I, const Values &a, Values &r) {
        float ray[3] = {(float)need_num(a, 0, "ray_to_latlon"), (float)need_num(a, 1, "ray_to_latlon"),
                        (float)need_num(a, 2, "ray_to_latlon")};
        double lat, lon;
        h_ray_to_latlon(*I.math, ray, &lat, &lon);
        r.push_back(Value::number(lat));
        r.push_back(Value::number(lon));
    });
    interp.register_builtin("plate_to_ray", [ctx](Interp &, const Values &a, Values &r) {
        int pi = h_trunc_to_int(need_num(a, 0, "plate_to_ray"));
        double u = need_num(a, 1, "plate_to_ray"), v = need_num(a, 2, "plate_to_ray");
        if (pi < 0 || pi >= ctx->numplates) { r.push_back(Value()); return; }       /* fisheye.c:1527-1530 */
        float ray[3];
        h_plate_uv_to_ray(ctx->plates[pi], u, v, ray);
        for (int i = 0; i < 3; ++i) r.push_back(Value::number((double)ray[i]));
    });
}

void lensprogram_free(LensProgram *p)
{
    if (!p) return;
    if (p->module) (void)hipModuleUnload(p->module);
    park_compile(p->pending);           // a compile still running must not stall the teardown
    delete p;
}

// LensProgram::emitted is keyed on the interpreter's activity count, which Interp::run / set_global move.  The translation unit is
// generated from the three callback roots as well (BK_HAS_GLOBE_PLATE and LF_globe_plate, which of the lens kernels exist), and a call
// that replaces a root WITHOUT running script code - bk_set_globe_plates, bk_clear_globe, bk_clear_lens - leaves the count where it is,
// bk_build's KeepActivity having rewound it to the very value the answer was remembered at: the answer is forgotten here instead, and
// the next generate_source / build_module_ready emits again (and re-arms KeepActivity at the count of that moment).
static void roots_changed(LensProgram *P)
{
    if (P) P->emitted.valid = false;
}

static void fill_plate(const MathLib &M, bk_plate &p, const double fwd[3], const double up[3], double fov_deg, bool *fov_ok)
{
    for (int j = 0; j < 3; ++j) p.forward[j] = (float)fwd[j];                  /* fisheye.c:1818 */
    for (int j = 0; j < 3; ++j) p.up[j] = (float)up[j];                        /* :1843 */
    h_cross(p.up, p.forward, p.right);                                          /* :1849 */
    h_cross(p.forward, p.right, p.up);                                          /* :1850 */
    p.fov = (float)(fov_deg * 3.14159265358979323846 / 180);                    /* :1858 */
    *fov_ok = p.fov > 0;                                                        /* :1861 */
    p.dist = (float)(0.5 / M.tan((double)(p.fov / 2)));                         /* :1868 */
}

}  // namespace bk

using bk::LensProgram;

// ---- globe ---------------------------------------------------------------------------------------------

extern "C" int bk_load_globe(bk_ctx *ctx, const char *src, size_t len, const char *chunkname)
{
    if (!ctx || !src) return BK_E_INVALID;
    LensProgram *P = bk::prog_of(ctx);
    Interp &I = P->interp;
    const std::string name = chunkname ? chunkname : "globe";
    // LUA_clear_globe, fisheye.c:1897-1903
    I.set_global("plates", Value());
    I.set_global("globe_plate", Value());
    ctx->numplates = 0;
    ctx->globe_valid = false;
    ctx->clear_debug_corners();                       // (a test's corner table was sized for the plates that are going)
    bk::seam_drop(ctx);                               // (the seam table was made for them, or set for them)
    P->globe_plate = Value();
    try {
        I.run(std::string(src, len), name);
        Value gp = I.get_global("globe_plate");
        if (gp.is_function()) P->globe_plate = gp;                              /* :1778-1782 */
        Value plates = I.get_global("plates");
        if (plates.t != Value::TABLE || plates.tab()->length() < 1)
            return ctx->fail(BK_E_SCRIPT, "plates must be an array of one or more elements");   /* :1788 */
        // lua_next order: array part, then the rest (:1796)
        Values items;
        items.append(plates.tab()->arr.data(), plates.tab()->arr.data() + plates.tab()->arr.size());
        for (auto &kv : plates.tab()->nhash) items.push_back(kv.second);
        for (auto &kv : plates.tab()->shash) items.push_back(kv.second);
        if (items.size() > BK_MAX_PLATES)
            return ctx->fail(BK_E_SCRIPT, "globe defines %zu plates; at most %d are supported (MAX_PLATES, fisheye.c:352)",
                             items.size(), BK_MAX_PLATES);
        int i = 0;
        for (const Value &plate : items) {
            double vec[2][3];
            static const char *vname[2] = {"forward", "up"};
            if (plate.t != Value::TABLE) return ctx->fail(BK_E_SCRIPT, "plate %d: not a table", i + 1);
            for (int k = 0; k < 2; ++k) {
                Value v = plate.tab()->get(Value::number(k + 1));
                if (v.t != Value::TABLE || v.tab()->length() != 3)
                    return ctx->fail(BK_E_SCRIPT, "plate %d: %s vector is not a 3d vector", i + 1, vname[k]);   /* :1804,1829 */
                for (int j = 0; j < 3; ++j) {
                    Value e = v.tab()->get(Value::number(j + 1));
                    if (e.t != Value::NUM)
                        return ctx->fail(BK_E_SCRIPT, "plate %d: %s vector: element %d not a number", i + 1, vname[k], j + 1);
                    vec[k][j] = e.n;
                }
            }
            Value fov = plate.tab()->get(Value::number(3));
            bool fov_ok = false;
            bk::fill_plate(*I.math, ctx->plates[i], vec[0], vec[1], fov.t == Value::NUM ? fov.n : 0.0, &fov_ok);
            if (!fov_ok) return ctx->fail(BK_E_SCRIPT, "plate %d: fov must > 0", i + 1);                       /* :1863 */
            ++i;
        }
        ctx->numplates = i;                                                     /* :1872 */
        ctx->globe_valid = true;
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "could not load globe: %s", e.what());
    }
    return BK_OK;
}

extern "C" int bk_get_globe(const bk_ctx *ctx, bk_plate plates[BK_MAX_PLATES], int *n)
{
    if (!ctx) return BK_E_INVALID;
    for (int i = 0; i < ctx->numplates; ++i) plates[i] = ctx->plates[i];
    if (n) *n = ctx->numplates;
    return BK_OK;
}

extern "C" int bk_set_globe_plates(bk_ctx *ctx, const bk_plate *plates, int numplates)
{
    if (!ctx || !plates || numplates < 1 || numplates > BK_MAX_PLATES) return BK_E_INVALID;
    for (int i = 0; i < numplates; ++i) ctx->plates[i] = plates[i];
    ctx->numplates = numplates;
    ctx->globe_valid = true;
    ctx->clear_debug_corners();
    bk::seam_drop(ctx);
    if (ctx->prog) { ctx->prog->globe_plate = Value(); bk::roots_changed(ctx->prog); }
    return BK_OK;
}

// ---- lens ------------------------------------------------------------------------------------------------

extern "C" int bk_load_lens(bk_ctx *ctx, const char *src, size_t len, const char *chunkname)
{
    if (!ctx || !src) return BK_E_INVALID;
    LensProgram *P = bk::prog_of(ctx);
    Interp &I = P->interp;
    const std::string name = chunkname ? chunkname : "lens";
    bk::seam_drop(ctx);                               // (globe and lens share one interpreter state: what globe_plate reads may change)
    // LUA_clear_lens, fisheye.c:1880-1894
    for (const char *g : {"map", "max_fov", "max_vfov", "lens_width", "lens_height", "lens_inverse", "lens_forward", "onload"})
        I.set_global(g, Value());
    I.set_global("numplates", Value::number((double)ctx->numplates));
    P->lens_valid = false;
    P->lens_inverse = P->lens_forward = Value();
    memset(&P->info, 0, sizeof P->info);
    try {
        I.run(std::string(src, len), name);
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "could not load lens: %s", e.what());
    }
    bk_lens_info &info = P->info;
    info.map_type = BK_MAP_NONE;
    Value inv = I.get_global("lens_inverse"), fwd = I.get_global("lens_forward");
    if (inv.is_function()) { P->lens_inverse = inv; info.has_inverse = 1; info.map_type = BK_MAP_INVERSE; }      /* :1688-1696 */
    if (fwd.is_function()) {                                                                                  /* :1699-1709 */
        P->lens_forward = fwd;
        info.has_forward = 1;
        if (info.map_type == BK_MAP_NONE) info.map_type = BK_MAP_FORWARD;
    }
    Value map = I.get_global("map");                                                                          /* :1712-1731 */
    if (map.t == Value::STR || map.t == Value::NUM) {
        std::string fn = I.tostring(map);
        if (fn == "lens_inverse") info.map_type = BK_MAP_INVERSE;
        else if (fn == "lens_forward") info.map_type = BK_MAP_FORWARD;
        else return ctx->fail(BK_E_SCRIPT, "Unsupported map function: %s", fn.c_str());
    }
    auto num_or_zero = [&](const char *g) { Value v = I.get_global(g); return v.t == Value::NUM ? v.n : 0.0; };
    info.max_fov = h_trunc_to_int(num_or_zero("max_fov"));                                                               /* :1733-1739 */
    info.max_vfov = h_trunc_to_int(num_or_zero("max_vfov"));
    info.lens_width = num_or_zero("lens_width");                                                              /* :1741-1747 */
    info.lens_height = num_or_zero("lens_height");
    Value onload = I.get_global("onload");                                                                    /* cmd_lens :1087-1095 */
    if (onload.t == Value::STR || onload.t == Value::NUM) snprintf(info.onload, sizeof info.onload, "%s", I.tostring(onload).c_str());
    P->lens_valid = true;
    return BK_OK;
}

// "not a valid lens" / "not a valid globe" (fisheye.c:1080-1083, 1157-1160): the host could not even
// read the script; the next bk_build then clears the map and reports the invalid state
extern "C" int bk_clear_lens(bk_ctx *ctx)
{
    if (!ctx) return BK_E_INVALID;
    bk::seam_drop(ctx);
    if (ctx->prog) { ctx->prog->lens_valid = false; ctx->prog->lens_inverse = ctx->prog->lens_forward = Value(); bk::roots_changed(ctx->prog); }
    return BK_OK;
}

extern "C" int bk_clear_globe(bk_ctx *ctx)
{
    if (!ctx) return BK_E_INVALID;
    ctx->globe_valid = false;
    ctx->numplates = 0;
    bk::seam_drop(ctx);
    if (ctx->prog) { ctx->prog->globe_plate = Value(); bk::roots_changed(ctx->prog); }
    return BK_OK;
}

extern "C" int bk_get_lens_info(const bk_ctx *ctx, bk_lens_info *out)
{
    if (!ctx || !out) return BK_E_INVALID;
    if (!ctx->prog || !ctx->prog->lens_valid) { memset(out, 0, sizeof *out); return BK_E_STATE; }
    *out = ctx->prog->info;
    return BK_OK;
}

// ---- callbacks on the host (calc_zoom only; per-pixel evaluation happens on the GPU) ---------------------

// LUAtoC_lens_forward, fisheye.c:1590-1632: 1 ok, 0 nil, -1 malformed
static int host_lens_forward(bk_ctx *ctx, const float ray[3], double *x, double *y)
{
    LensProgram *P = ctx->prog;
    Values r = P->interp.call(P->lens_forward, Values{Value::number((double)ray[0]), Value::number((double)ray[1]),
                                                      Value::number((double)ray[2])});
    if (r.size() == 2) {
        if (r[0].t == Value::NUM && r[1].t == Value::NUM) { *x = r[0].n; *y = r[1].n; return 1; }
        ctx->fail(BK_E_SCRIPT, "lens_forward returned a non-number value for x,y");
        return -1;
    }
    if (r.size() == 1) {
        if (r[0].t == Value::NIL) return 0;
        ctx->fail(BK_E_SCRIPT, "lens_forward returned a single non-nil value");
        return -1;
    }
    ctx->fail(BK_E_SCRIPT, "lens_forward returned %zu values instead of 2", r.size());
    return -1;
}

extern "C" int bk_calc_zoom(bk_ctx *ctx, double *scale_out)
{
    if (!ctx) return BK_E_INVALID;
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid) return ctx->fail(BK_E_STATE, "no valid lens");
    if (ctx->W <= 0 || ctx->H <= 0) return ctx->fail(BK_E_STATE, "bk_calc_zoom: call bk_resize first");
    const bk_lens_info &L = P->info;
    double scale = -1;                                                                   /* :1296 */
    try {
        if (ctx->zoom_type == BK_ZOOM_FOV || ctx->zoom_type == BK_ZOOM_VFOV) {
            if (L.max_fov <= 0 || L.max_vfov <= 0)
                return ctx->fail(BK_E_ZOOM, "max_fov & max_vfov not specified, try \"f_cover\"");            /* :1303 */
            if (ctx->zoom_type == BK_ZOOM_FOV && ctx->zoom_fov > L.max_fov)
                return ctx->fail(BK_E_ZOOM, "fov must be less than %d", L.max_fov);                           /* :1307 */
            if (ctx->zoom_type == BK_ZOOM_VFOV && ctx->zoom_fov > L.max_vfov)
                return ctx->fail(BK_E_ZOOM, "vfov must be less than %d", L.max_vfov);                         /* :1311 */
            if (!L.has_forward)
                return ctx->fail(BK_E_ZOOM, "Please specify a forward mapping function in your script for FOV scaling");   /* :1343 */
            float ray[3];
            double x = 0, y = 0;
            const double fovr = ctx->zoom_fov * 3.14159265358979323846 / 180;                                 /* :1319 */
            if (ctx->zoom_type == BK_ZOOM_FOV) bk::h_latlon_to_ray(*P->interp.math, 0, fovr * 0.5, ray);       /* :1321 */
            else bk::h_latlon_to_ray(*P->interp.math, fovr * 0.5, 0, ray);                                     /* :1331 */
            const int st = host_lens_forward(ctx, ray, &x, &y);
            if (st == -1) return BK_E_SCRIPT;
            if (st == 0) return ctx->fail(BK_E_ZOOM, "ray_to_xy did not return a valid r value for determining FOV scale");
            scale = ctx->zoom_type == BK_ZOOM_FOV ? x / (ctx->W * 0.5) : y / (ctx->H * 0.5);                   /* :1323, 1333 */
        } else if (ctx->zoom_type == BK_ZOOM_CONTAIN || ctx->zoom_type == BK_ZOOM_COVER) {
            const double fit_w = L.lens_width / ctx->W, fit_h = L.lens_height / ctx->H;                        /* :1349-1350 */
            const bool wp = L.lens_width > 0, hp = L.lens_height > 0;
            if (!wp && hp) scale = fit_h;
            else if (wp && !hp) scale = fit_w;
            else if (!wp && !hp)
                return ctx->fail(BK_E_ZOOM, "neither lens_height nor lens_width are valid/specified.  Try f_fov instead.");
            else {
                const double lens_aspect = L.lens_width / L.lens_height;
                const double screen_aspect = (double)ctx->W / ctx->H;
                const bool lens_wider = lens_aspect > screen_aspect;
                if (ctx->zoom_type == BK_ZOOM_CONTAIN) scale = lens_wider ? fit_w : fit_h;
                else scale = lens_wider ? fit_h : fit_w;
            }
        }
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "lens_forward failed: %s", e.what());
    }
    // (as the reference writes it: a NaN scale - a lens_forward that returns NaN - is NOT rejected and builds an empty map)
    if (scale <= 0) return ctx->fail(BK_E_ZOOM, "init returned a scale of %f, which is  <= 0", scale);          /* :1380 */
    ctx->scale = scale;
    if (scale_out) *scale_out = scale;
    return BK_OK;
}

// ---- the lens module: generated source -> code object (bk_modules.cpp) -> loaded kernels --------------------------------

static std::string target_arch(bk_ctx *ctx)
{
    hipDeviceProp_t prop;
    if (ctx->device >= 0 && hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.gcnArchName[0])
        return std::string("--offload-arch=") + prop.gcnArchName;
    return "--offload-arch=gfx950";
}

static int load_module(bk_ctx *ctx, LensProgram *P, const std::string &source, const CodeResult &cr)
{
    if (cr.rc != BK_OK) return ctx->fail(cr.rc, "%s", cr.log.c_str());
    if (P->module) { (void)hipModuleUnload(P->module); P->module = nullptr; }
    P->k_inverse = P->k_corners = P->k_quads = P->k_resolve = P->k_tiles = nullptr;
    P->module_from_cache = cr.from_disk;
    if (ctx->device < 0) {              // host-only context: compiling is all we can do
        P->module_source = source;
        return BK_OK;
    }
    BK_HIP(ctx, hipModuleLoadData(&P->module, cr.code->data()));
    (void)hipModuleGetFunction(&P->k_inverse, P->module, "bk_build_inverse");
    (void)hipModuleGetFunction(&P->k_corners, P->module, "bk_forward_corners");
    (void)hipModuleGetFunction(&P->k_quads, P->module, "bk_forward_quads");
    (void)hipModuleGetFunction(&P->k_resolve, P->module, "bk_forward_resolve");
    if (hipModuleGetFunction(&P->k_tiles, P->module, "bk_forward_tiles") != hipSuccess) P->k_tiles = nullptr;   // (absent under a globe_plate script)
    (void)hipGetLastError();
    P->module_source = source;
    return BK_OK;
}

int compile_module(bk_ctx *ctx, LensProgram *P, const std::string &source)
{
    if (P->module_source == source && (P->module || ctx->device < 0)) return BK_OK;
    return load_module(ctx, P, source, compile_code(source, target_arch(ctx)));
}

// bk_build with asynchronous compilation (bk_set_async_compile): BK_PENDING while hiprtc works on another thread
static int compile_module_async(bk_ctx *ctx, LensProgram *P, const std::string &source)
{
    if (P->module_source == source && P->module) return BK_OK;
    const std::string arch = target_arch(ctx);
    if (P->pending.valid() && P->pending_source == source) {
        if (P->pending.wait_for(std::chrono::seconds(0)) != std::future_status::ready) return BK_PENDING;
        CodeResult cr = P->pending.get();
        P->pending_source.clear();
        P->pending = std::shared_future<::CodeResult>();
        return load_module(ctx, P, source, cr);
    }
    CodeResult cr = cached_code(source, arch);                      // memory / disk: no reason to wait a frame
    if (cr.code) return load_module(ctx, P, source, cr);
    park_compile(P->pending);                                       // (an older source's compile finishes on its own thread)
    P->pending_source = source;
    P->pending = std::async(std::launch::async, [source, arch]() { return compile_code(source, arch); }).share();
    return BK_PENDING;
}

// the asynchronous-compile gate of bk_build / bk_multi_build: is the module for the current lens + globe there?
int bk::build_module_ready(bk_ctx *ctx)
{
    LensProgram *P = ctx->prog;
    if (!(ctx->async_compile && P && P->lens_valid && ctx->globe_valid && P->info.map_type != BK_MAP_NONE)) return BK_OK;
    // a lens that still has to go through hiprtc (0.2-1.1 s): compile on another thread and leave the previous
    // lensmap untouched until the module is there - the caller keeps drawing with it and calls bk_build again
    std::string psrc;
    bk::EmitRequest rq;
    rq.interp = &P->interp; rq.lens_inverse = P->lens_inverse; rq.lens_forward = P->lens_forward; rq.globe_plate = P->globe_plate;
    if (P->emitted.valid && P->emitted.activity == P->interp.activity && P->emitted.libm_rel == bk::g_debug.libm_rel_log2) {
        if (!P->emitted.refused.empty()) return BK_OK;                                       // (a host-path lens: nothing to compile)
        psrc = P->emitted.src;                                                                // (generate_source's answer still stands)
    } else
    try { psrc = bk::emit_build_source(rq); } catch (const LuaError &) { return BK_OK; }      // (reported by the normal path)
    // A module that is ready gets LOADED here (hipModuleLoadData / hipModuleGetFunction): that has to happen on the context's own
    // device, whatever device the calling thread was left on - bk_multi_build asks on behalf of stripe 0 right after a
    // bk_multi_apply whose loop ended on the LAST stripe's device, and kernels loaded there would later be launched on stripe 0's
    // stream (invalid device function on a node with more than one GPU).  The caller's device is put back.
    int prev = -1;
    const bool switched = ctx->device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != ctx->device && hipSetDevice(ctx->device) == hipSuccess;
    const int rc = compile_module_async(ctx, P, psrc) == BK_PENDING ? BK_PENDING : BK_OK;
    if (switched) (void)hipSetDevice(prev);
    return rc;
}

extern "C" int bk_set_async_compile(bk_ctx *ctx, int on)
{
    if (!ctx) return BK_E_INVALID;
    ctx->async_compile = on != 0;
    return BK_OK;
}

/* `refused` (nullable): a script whose callbacks use a construct the emitter does not turn into GPU code (recursion, tables made at
 * run time, functions as values, strings ...) is not an error for a caller that passes it - the text of the refusal comes back in
 * it, *out stays empty, and bk_build evaluates the callbacks with the host interpreter instead (build_on_host). */
int generate_source(bk_ctx *ctx, LensProgram *P, std::string *out, std::string *refused)
{
    bk::EmitRequest rq;
    rq.interp = &P->interp;
    rq.lens_inverse = P->lens_inverse;
    rq.lens_forward = P->lens_forward;
    rq.globe_plate = P->globe_plate;
    if (refused) refused->clear();
    if (P->emitted.valid && P->emitted.activity == P->interp.activity && P->emitted.libm_rel == bk::g_debug.libm_rel_log2 &&
        (refused || P->emitted.refused.empty())) {
        *out = P->emitted.src;
        if (refused) *refused = P->emitted.refused;
        return BK_OK;
    }
    P->emitted.valid = false;
    const auto remember = [&](const std::string &src, const std::string &why) {
        P->emitted.src = src; P->emitted.refused = why;
        P->emitted.activity = P->interp.activity; P->emitted.libm_rel = bk::g_debug.libm_rel_log2;
        // callbacks that change nothing a script can see: bk_build may run them (calc_zoom, the flagged entries) and keep this answer
        try { std::string which; P->emitted.stateless = !bk::callbacks_carry_state(rq, &which); } catch (const LuaError &) { P->emitted.stateless = false; }
        P->emitted.valid = true;
    };
    try {
        *out = bk::emit_build_source(rq);
        // test hook: a wider assumed libm discrepancy (tests pair it with bk_set_host_math(ctx, n): the host interpreter on a
        // stand-in libm 2^-n away from bkm.h), so that the flag -> host fix-up path is exercised on thousands of pixels
        if (const int n = bk::g_debug.libm_rel_log2)
            if (n >= 8 && n <= 52) *out = "#define BK_LIBM_REL 0x1p-" + std::to_string(n) + "\n" + *out;
    } catch (const LuaError &e) {
        if (refused && strstr(e.what(), "GPU callback")) {          // (bk_emit.cpp's `unsupported`, and its two "assigned inside a GPU callback but holds a ..." refusals)
            out->clear();
            *refused = e.what();
            remember(*out, *refused);
            return BK_OK;
        }
        return ctx->fail(BK_E_SCRIPT, "%s", e.what());
    }
    P->last_source = *out;
    remember(*out, std::string());
    return BK_OK;
}

#if BK_DEBUG_API
// debug / test hook: the generated HIP translation unit for the current lens + globe
extern "C" int bk_debug_kernel_source(bk_ctx *ctx, char *buf, size_t cap, size_t *needed, int compile)
{
    if (!ctx) return BK_E_INVALID;
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid) return ctx->fail(BK_E_STATE, "no valid lens");
    std::string src;
    if (int r = generate_source(ctx, P, &src)) return r;
    if (needed) *needed = src.size() + 1;
    if (buf && cap) snprintf(buf, cap, "%s", src.c_str());
    if (compile) return compile_module(ctx, P, src);
    return BK_OK;
}
#endif

#if BK_DEBUG_API
// debug / test hook: evaluate a callback with the HOST interpreter (the same AST the GPU code was
// generated from).  which: 0 = lens_inverse(x,y), 1 = lens_forward(x,y,z), 2 = globe_plate(x,y,z)
extern "C" int bk_debug_eval(bk_ctx *ctx, int which, const double *args, int nargs, double *out, int *nout)
{
    if (!ctx || !ctx->prog) return BK_E_INVALID;
    LensProgram *P = ctx->prog;
    const Value &f = which == 0 ? P->lens_inverse : which == 1 ? P->lens_forward : P->globe_plate;
    if (!f.is_function()) return ctx->fail(BK_E_STATE, "callback not defined");
    try {
        Values a;
        for (int i = 0; i < nargs; ++i) a.push_back(Value::number(args[i]));
        P->interp.steps = 0;                                         // (the budget is per call, as in HostEval::call: one runaway evaluation must not fail the next)
        Values r = P->interp.call(f, a);
        *nout = (int)r.size();
        for (size_t i = 0; i < r.size() && i < 8; ++i) out[i] = r[i].t == Value::NUM ? r[i].n : __builtin_nan("");
        if (r.size() == 1 && r[0].t == Value::NIL) *nout = -1;       // a single nil
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "%s", e.what());
    }
    return BK_OK;
}
#endif

#if BK_DEBUG_API
/* test hook: 1 if the current lens module came from the BLINKY_HIP_CACHE directory instead of hiprtc */
extern "C" int bk_debug_module_from_cache(const bk_ctx *ctx) { return ctx && ctx->prog && ctx->prog->module_from_cache ? 1 : 0; }
#endif

extern "C" int bk_set_host_math(bk_ctx *ctx, int portable)
{
    if (!ctx) return BK_E_INVALID;
#if BK_DEBUG_API
    if (portable >= 2) {            // the test suite's stand-in libms (include/blinky_hip_debug.h)
        bk::prog_of(ctx)->interp.math = &math_perturbed(ldexp(1.0, -(portable & 63)), portable >> 6);
        return BK_OK;
    }
#else
    if (portable >= 2) return ctx->fail(BK_E_INVALID, "bk_set_host_math: %d is a test mode of debug-API builds", portable);
#endif
    bk::prog_of(ctx)->interp.math = portable ? &math_portable() : &math_platform();
    return BK_OK;
}

extern "C" const char *bk_script_console(bk_ctx *ctx) { return ctx && ctx->prog ? ctx->prog->console.c_str() : ""; }
