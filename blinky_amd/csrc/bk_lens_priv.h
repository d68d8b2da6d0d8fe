// bk_lens_priv.h -- what bk_lens.cpp (scripts, zoom, the lens module) and bk_build.cpp (every build path) share.
#pragma once

#include <future>
#include <string>

#include "bk_internal.h"
#include "bk_lua.h"
#include "bk_modules.h"

/* (int)double as the reference's x86-64 build converts it (cvttsd2si): NaN and out-of-range values become INT_MIN - where the
 * reference assigns a Lua number to an int (fisheye.c:1522, 1734, 1738) the C language leaves that case undefined */
static inline int h_trunc_to_int(double v)
{
    if (!(v > -2147483649.0 && v < 2147483648.0)) return (int)0x80000000;
    return (int)v;
}

namespace bk {

struct LensProgram {
    bklua::Interp interp;
    // lens (fisheye.c:379-451 + lua_refs 328-332)
    bool lens_valid = false;
    bk_lens_info info{};
    bklua::Value lens_inverse, lens_forward, globe_plate;
    // compiled build kernels, keyed by the generated source text
    std::string module_source;
    hipModule_t module = nullptr;
    bool module_from_cache = false;      // the last compile_module() loaded its code object from BLINKY_HIP_CACHE
    hipFunction_t k_inverse = nullptr, k_corners = nullptr, k_quads = nullptr, k_resolve = nullptr, k_tiles = nullptr;
    std::shared_future<::CodeResult> pending;     // bk_set_async_compile: hiprtc running on another thread ...
    std::string pending_source;                      // ... for this generated source
    // generate_source's last answer and the interpreter activity it was given at: emitting the translation unit walks the callbacks
    // (16 us for winkel2, 43 for panini, 280 for quincuncial on the build host) and was done again on every bk_build
    struct { bool valid = false; unsigned long long activity = 0; int libm_rel = 0; bool stateless = false; std::string src, refused; } emitted;
    bool fwd_needs_host = false;  // the last forward build flagged entries for the host: the next one stops after each pass again
    std::string last_source;      // for bk_debug_kernel_source
    std::string console;          // print() output of the scripts

    explicit LensProgram(bk_ctx *ctx);
};

static inline LensProgram *prog_of(bk_ctx *ctx)
{
    if (!ctx->prog) ctx->prog = new LensProgram(ctx);
    return ctx->prog;
}

// ---- host versions of the converters (fisheye.c:1184-1214), on the portable libm ----------------
static inline void h_vector_ma(const float *a, float scale, const float *b, float *c)
{
    c[0] = a[0] + scale * b[0];
    c[1] = a[1] + scale * b[1];
    c[2] = a[2] + scale * b[2];
}
static inline void h_vector_normalize(float *v)
{
    float length = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    length = (float)__builtin_sqrt((double)length);
    if (length) {
        float ilength = 1 / length;
        v[0] *= ilength;
        v[1] *= ilength;
        v[2] *= ilength;
    }
}
static inline void h_latlon_to_ray(const bklua::MathLib &M, double lat, double lon, float *ray)
{
    double clat = M.cos(lat);
    ray[0] = (float)(M.sin(lon) * clat);
    ray[1] = (float)M.sin(lat);
    ray[2] = (float)(M.cos(lon) * clat);
}
static inline void h_ray_to_latlon(const bklua::MathLib &M, const float *ray, double *lat, double *lon)
{
    *lon = M.atan2((double)ray[0], (double)ray[2]);
    *lat = M.atan2((double)ray[1], M.sqrt((double)(ray[0] * ray[0] + ray[2] * ray[2])));
}

static inline void h_plate_uv_to_ray(const bk_plate &p, double u, double v, float *ray)
{
    u -= 0.5;
    v -= 0.5;
    v = -v;
    ray[0] = ray[1] = ray[2] = 0;
    h_vector_ma(ray, p.dist, p.forward, ray);
    h_vector_ma(ray, (float)u, p.right, ray);
    h_vector_ma(ray, (float)v, p.up, ray);
    h_vector_normalize(ray);
}
static inline void h_cross(const float *v1, const float *v2, float *cross)            /* mathlib.c:389 */
{
    cross[0] = v1[1] * v2[2] - v1[2] * v2[1];
    cross[1] = v1[2] * v2[0] - v1[0] * v2[2];
    cross[2] = v1[0] * v2[1] - v1[1] * v2[0];
}

}  // namespace bk

#pragma GCC visibility push(hidden)
/* the generated translation unit of the current lens + globe (bk_lens.cpp).  `refused` (nullable): a script whose callbacks the emitter
 * does not turn into GPU code is not an error for a caller that passes it - the refusal comes back in it and *out stays empty */
int generate_source(bk_ctx *ctx, bk::LensProgram *P, std::string *out, std::string *refused = nullptr);
// the kernels of `source` compiled (or found in a cache) and loaded into P->module
int compile_module(bk_ctx *ctx, bk::LensProgram *P, const std::string &source);
#pragma GCC visibility pop
