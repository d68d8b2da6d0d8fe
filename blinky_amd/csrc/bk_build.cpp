// bk_build.cpp -- every lensmap build path: the device passes (inverse, forward) with the host re-derivation of the entries they
// flag, the host builds for scripts the kernels cannot run, and the build-side debug hooks.  Mirrors fisheye.c's create_lensmap
// (2367-2397); scripts, zoom and the lens module are bk_lens.cpp.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>

#include "bk_build_params.h"
#include "bk_emit.h"
#include "bk_hostpool.h"
#include "bk_lens_priv.h"
#include "bkm.h"

using namespace bklua;
using bk::LensProgram;

// ---- build -----------------------------------------------------------------------------------------------

static void fill_params(bk_ctx *ctx, BkBuildParams *bp)
{
    memset(bp, 0, sizeof *bp);
    bp->W = ctx->W; bp->H = ctx->H;
    bp->row0 = ctx->row0; bp->rows = ctx->rows();
    bp->ps = ctx->ps; bp->gp = ctx->gp; bp->ph = ctx->ph;
    bp->numplates = ctx->numplates;
    bp->has_globe_plate = ctx->prog->globe_plate.is_function();
    bp->scale = ctx->scale;
    bp->inv_scale_up = 1.0 / __builtin_fabs(ctx->scale) * (1.0 + 0x1p-50);
    // set_lensmap_grid constants, fisheye.c:1938-1948 (same double operations)
    const double block_size = ctx->rubix.pad + ctx->rubix.cell;
    const double num_units = ctx->rubix.numcells * block_size + ctx->rubix.pad;
    bp->rubix_block = block_size;
    bp->rubix_pad = ctx->rubix.pad;
    bp->rubix_unit_px = (double)ctx->ps / num_units;
    if (ctx->ps <= 32 * (int)(sizeof bp->grid_bits / sizeof bp->grid_bits[0])) {
        const double key[4] = {(double)ctx->ps, (double)ctx->rubix.numcells, ctx->rubix.cell, ctx->rubix.pad};
        if (memcmp(key, ctx->grid_cache_key, sizeof key) != 0) {
            memset(ctx->grid_cache, 0, sizeof ctx->grid_cache);
            for (int p = 0; p < ctx->ps; ++p)            /* fisheye.c:1950-1957; division and fmod are exact operations */
                if (__builtin_fmod((double)p / bp->rubix_unit_px, bp->rubix_block) < bp->rubix_pad) ctx->grid_cache[p >> 5] |= 1u << (p & 31);
            memcpy(ctx->grid_cache_key, key, sizeof key);
        }
        static_assert(sizeof ctx->grid_cache == sizeof bp->grid_bits, "one bitmap");
        memcpy(bp->grid_bits, ctx->grid_cache, sizeof bp->grid_bits);
        bp->grid_n = ctx->ps;
    }
    for (int i = 0; i < ctx->numplates; ++i) {
        const bk_plate &p = ctx->plates[i];
        BkPlateDev &d = bp->plates[i];
        memcpy(d.forward, p.forward, 12); memcpy(d.right, p.right, 12); memcpy(d.up, p.up, 12);
        d.fov = p.fov; d.dist = p.dist;
        d.dist64 = 0.5 / ctx->prog->interp.math->tan((double)(p.fov / 2));      /* fisheye.c:2060 */
    }
    bp->offsets = ctx->d_offsets;
    bp->tints = ctx->d_tints;
    bp->subtexel = ctx->d_subtexel;               // (null unless bk_set_subtexel is on: the kernel then stores nothing)
    bp->display = ctx->d_display;
    bp->err = ctx->d_display + BK_MAX_PLATES;
    bp->flag_count = (unsigned int *)(ctx->d_display + BK_MAX_PLATES + 1);
    bp->first_bad = (unsigned int *)(ctx->d_display + BK_MAX_PLATES + 2);
    bp->flag_list = ctx->d_flag_list;
    bp->flag_cap = (unsigned int)ctx->flag_cap;
}

static const char *err_text(int bits)
{
    if (bits & BK_ERR_LOOP) return "a lens callback exceeded the per-pixel iteration budget (infinite loop?)";
    if (bits & BK_ERR_ARITH) return "a lens callback performed arithmetic on a non-number (nil?)";
    if (bits & BK_ERR_COMPARE) return "a lens callback compared non-numbers with < or <=";
    if (bits & BK_ERR_INDEX) return "a lens callback stored outside a table's bounds";
    if (bits & BK_ERR_RESULT) return "a lens callback returned a malformed result (not 3 numbers / 2 numbers / a single nil)";
    return "unknown device error";
}

// ---- host re-evaluation of the entries a build flagged ------------------------------------------------------
// The device evaluates the callbacks on bkm.h; the reference's Lua VM calls the platform libm.  The kernels
// flag every pixel / texel corner / texel whose DISCRETE outcome could depend on the last bits of a
// transcendental (bk_device_rt.h) - a handful per 4K map - and the functions below re-derive exactly those
// with this context's host interpreter (platform libm unless bk_set_host_math says otherwise: the same
// evaluator calc_zoom and the globe loader use), restating fisheye.c's float/double tail, and patch the table.
namespace {

float h_dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }     /* mathlib.h:70 */
/* who evaluates: the context's interpreter, or a per-thread copy of it (Interp::clone) */
struct HostEval {
    Interp *I;
    Value lens_inverse, lens_forward, globe_plate;
    Values call(const Value &f, const Values &a) { I->steps = 0; return I->call(f, a); }
};

/* ray_to_plate_index, fisheye.c:2023-2050 (same out-of-range handling as the kernel's) */
int h_ray_to_plate_index(HostEval &E, const BkBuildParams &bp, const float *ray)
{
    if (E.globe_plate.is_function()) {
        Values r = E.call(E.globe_plate, Values{Value::number((double)ray[0]), Value::number((double)ray[1]),
                                                Value::number((double)ray[2])});
        if (r.empty() || r.back().t != Value::NUM) return -1;
        const double d = r.back().n;
        if (!(d > -2147483648.0 && d < 2147483647.0)) return -1;
        const int plate = (int)__builtin_rint(d);
        if (plate < 0 || plate >= bp.numplates) return -1;
        return plate;
    }
    int plate_index = 0;
    double max_dp = -2;
    for (int i = 0; i < bp.numplates; ++i) {
        const double dp = (double)h_dot3(ray, bp.plates[i].forward);
        if (dp > max_dp) { max_dp = dp; plate_index = i; }
    }
    return plate_index;
}

bool h_offgrid(const BkBuildParams &bp, int px, int py)                                                /* fisheye.c:1922-1960 */
{
    const double ux = (double)px / bp.rubix_unit_px, uy = (double)py / bp.rubix_unit_px;
    return !(__builtin_fmod(ux, bp.rubix_block) < bp.rubix_pad || __builtin_fmod(uy, bp.rubix_block) < bp.rubix_pad);
}

/* one pixel of resume_lensmap_inverse (fisheye.c:2084-2124, 1545-1588, 1995-2013); o = index inside the owned stripe; *sub = where inside
 * the texel the ray landed (what :1988 drops; bk_inverse_entry's three lines), 0x8080 for an entry that names none */
void h_inverse_entry(HostEval &E, const BkBuildParams &bp, uint32_t o, uint32_t *off, uint8_t *tint, uint16_t *sub,
                     int *plate_shown, int *err)
{
    *off = BK_NULL_OFFSET; *tint = 255; *sub = 0x8080; *plate_shown = -1;
    const int lyl = (int)(o / (uint32_t)bp.W), lx = (int)(o - (uint32_t)lyl * (uint32_t)bp.W), ly = bp.row0 + lyl;
    const double y = (double)(-(ly - bp.H / 2)) * bp.scale, x = (double)(lx - bp.W / 2) * bp.scale;
    Values r = E.call(E.lens_inverse, Values{Value::number(x), Value::number(y)});
    if (r.size() == 3 && r[0].t == Value::NUM && r[1].t == Value::NUM && r[2].t == Value::NUM) {
        float ray[3] = {(float)r[0].n, (float)r[1].n, (float)r[2].n};
        bk::h_vector_normalize(ray);
        const int plate = h_ray_to_plate_index(E, bp, ray);
        if (plate < 0) return;
        const BkPlateDev &p = bp.plates[plate];
        const double px_ = (double)h_dot3(p.right, ray), py_ = (double)h_dot3(p.up, ray), pz_ = (double)h_dot3(p.forward, ray);
        const double u = px_ / pz_ * p.dist64 + 0.5, v = -py_ / pz_ * p.dist64 + 0.5;
        if (u >= 0 && u <= 1 && v >= 0 && v <= 1) {
            const double us = u * bp.ps, vs = v * bp.ps;
            const int px = h_trunc_to_int(us), py = h_trunc_to_int(vs);
            if (px >= 0 && px < bp.ps && py >= 0 && py < bp.ps) {
                *plate_shown = plate;
                *off = bk_texel_offset((unsigned)bp.gp, (unsigned)bp.ph, (unsigned)plate, (unsigned)px, (unsigned)py);
                if (h_offgrid(bp, px, py)) *tint = (uint8_t)plate;
                *sub = (uint16_t)((int)((us - (double)px) * 256.0) | (int)((vs - (double)py) * 256.0) << 8);      /* exact: 0 <= us - px < 1 */
            }
        }
    } else if (!(r.size() == 1 && r[0].t == Value::NIL)) {
        *err |= BK_ERR_RESULT;
    }
}

/* one texel corner of the forward build: uv_to_screen, fisheye.c:2227-2243 */
void h_corner_entry(bk_ctx *ctx, HostEval &E, const BkBuildParams &bp, uint32_t id, int *sx, int *sy, uint8_t *ok, int *err)
{
    const uint32_t n1 = (uint32_t)bp.ps + 1u;
    const uint32_t plate = id / (n1 * n1), rem = id - plate * n1 * n1, j = rem / n1, i = rem - j * n1;
    const double u = ((double)i - 0.5) / bp.ps, v = ((double)j - 0.5) / bp.ps;
    float ray[3];
    bk::h_plate_uv_to_ray(ctx->plates[plate], u, v, ray);
    *sx = 0; *sy = 0; *ok = 0;
    Values r = E.call(E.lens_forward, Values{Value::number((double)ray[0]), Value::number((double)ray[1]),
                                              Value::number((double)ray[2])});
    if (r.size() == 2 && r[0].t == Value::NUM && r[1].t == Value::NUM) {
        *sx = h_trunc_to_int(r[0].n / bp.scale + (double)(bp.W / 2));
        *sy = h_trunc_to_int(-r[1].n / bp.scale + (double)(bp.H / 2));
        *ok = 1;
    } else if (!(r.size() == 1 && r[0].t == Value::NIL)) {
        *err |= BK_ERR_RESULT;
    }
}

/* forward build: does the ray through texel `id` select its own plate (fisheye.c:2193-2196) */
bool h_texel_owns(bk_ctx *ctx, HostEval &E, const BkBuildParams &bp, uint32_t id)
{
    const uint32_t ps = (uint32_t)bp.ps, plate = id / (ps * ps), rem = id - plate * ps * ps, py = rem / ps, px = rem - py * ps;
    float ray[3];
    bk::h_plate_uv_to_ray(ctx->plates[plate], (double)px / bp.ps, (double)py / bp.ps, ray);
    return (int)plate == h_ray_to_plate_index(E, bp, ray);
}

/* the flag list (records of four words, [0] = entry id) in ascending id order: the order the reference's scan meets the
 * entries in (fisheye.c:2084-2124), which is also what keeps a script's own caches warm - eckert4 solves its outline once
 * per ROW and remembers it in globals; met in the arbitrary order the kernel appended them every flagged pixel would solve
 * it again (20 Newton steps), an order of magnitude more host time on the rows it flags whole */
void sort_flagged(std::vector<uint32_t> &rec)
{
    const size_t n = rec.size() / 4;
    if (n < 2) return;
    bool sorted = true;
    for (size_t i = 1; i < n && sorted; ++i) sorted = rec[4 * (i - 1)] <= rec[4 * i];
    if (sorted) return;
    std::vector<uint64_t> key(n), tmp(n);
    for (size_t i = 0; i < n; ++i) key[i] = ((uint64_t)rec[4 * i] << 32) | (uint64_t)i;
    if (n < 4096) std::sort(key.begin(), key.end());
    else {
        for (int shift = 32; shift < 64; shift += 11) {           // LSD radix on the id, 11 bits a pass (stable)
            size_t count[2049] = {0};
            for (size_t i = 0; i < n; ++i) ++count[((key[i] >> shift) & 2047u) + 1];
            for (int b = 0; b < 2048; ++b) count[b + 1] += count[b];
            for (size_t i = 0; i < n; ++i) tmp[count[(key[i] >> shift) & 2047u]++] = key[i];
            key.swap(tmp);
        }
    }
    std::vector<uint32_t> out(rec.size());
    for (size_t i = 0; i < n; ++i) memcpy(&out[4 * i], &rec[4 * (size_t)(key[i] & 0xFFFFFFFFu)], 16);
    rec.swap(out);
}

/* fn(E, i) for i in [0, n): on the context's interpreter when the list is short, otherwise on the pool's workers, each
 * on its own deep copy of the interpreter state; the workers take runs of consecutive entries from a shared counter (the
 * entries cost very different amounts - a nil-test that fails at once, a Newton iteration - so equal static shares leave
 * most workers waiting for the unluckiest).  The first script error any worker meets is rethrown here. */
template <typename Fn>
void for_each_flagged(LensProgram *P, size_t n, Fn fn)
{
    // (never on the context's own interpreter: a callback that assigns script globals - fahey's `lat`, `lon` - would leave them
    //  changed, the next build's generated source would carry different initial values for them, and the lens would go through
    //  hiprtc again for nothing: the 490 ms second build of fahey in round 2's tables)
    if (!n) return;                                 // (nothing flagged - most builds: no copy of the interpreter, 30 us at 4K panini)
    const Values roots_in{P->lens_inverse, P->lens_forward, P->globe_plate};
    const size_t nthreads = n >= 256 ? std::max<size_t>(1, std::min(bk::HostPool::get().size(), n / 96)) : 1;
    const size_t run = std::max<size_t>(32, std::min<size_t>(2048, n / (nthreads * 6)));
    std::vector<std::string> errors(nthreads);
    bk::pool_runs(n, run, nthreads, [&](size_t t, bk::Runs &runs) {
        try {
            // every worker copies the interpreter for itself (the original is only read meanwhile)
            Values roots;
            std::unique_ptr<Interp> mine = P->interp.clone(roots_in, &roots);
            HostEval ev{mine.get(), roots[0], roots[1], roots[2]};
            for (size_t first, count; runs.next(&first, &count);)
                for (size_t i = first; i < first + count; ++i) fn(ev, i);
        } catch (const LuaError &e) { errors[t] = e.what(); }
    });
    for (const std::string &e : errors) if (!e.empty()) throw LuaError(e);
}

/* call(first, count) over [0, n) in runs of consecutive entries, on a few pool workers: the compiled host module answers an
 * entry in a fraction of a microsecond, so a handful of threads is plenty */
template <typename Call>
void hostmod_runs(size_t n, Call call)
{
    const size_t run = n < 65536 ? 128 : 512;       // (short lists in short runs: the last one to finish decides)
    bk::HostPool &pool = bk::HostPool::get();
    // (two runs per worker at least; r6: the cap was 48 below 200 K entries - waking more sleepers than that cost more than they brought
    //  while every one of them was waited for; measured at 4K: quincuncial's 20 132 entries 0.67-0.94 -> 0.49-0.55 ms, eckert4's 7 707 0.13 -> 0.12,
    //  winkeltripel's 10 431 0.50 -> 0.40-0.58: what is left is the sleepers' wake-up, one after the other)
    const size_t nthreads = n < 2 * run ? 1 : std::min<size_t>(std::min<size_t>(pool.size(), (n + 2 * run - 1) / (2 * run)), 128);
    bk::pool_runs(n, run, nthreads, [&](size_t, bk::Runs &runs) {
        for (size_t first, count; runs.next(&first, &count);) call(first, count);
    });
}

}  // namespace

/* the compiled host module to re-derive flagged entries with, or nullptr: the interpreter does it (host math switched away
 * from the platform libm, no compiler on this machine, still compiling, switched off) */
static HostModuleP fixup_module(LensProgram *P, const std::string &source)
{
    if (bk::g_debug.host_module == 2) return nullptr;
    if (P->interp.math != &math_platform()) return nullptr;
    return host_module_for(source, bk::g_debug.host_module == 1);
}

// a pass's counters at bk_ctx::d_display: display flags, error bits, flagged-entry count, first malformed result
constexpr int kNumCounters = BK_MAX_PLATES + 3;

/* the flag list and the pinned counters of the passes below (room for a forward build's two sets) */
static int alloc_flag_buffers(bk_ctx *ctx)
{
    if (!ctx->d_flag_list) {
        BK_HIP(ctx, hipMalloc((void **)&ctx->d_flag_list, (size_t)65536 * 4 * sizeof(uint32_t)));
        ctx->flag_cap = 65536;
    }
    if (!ctx->h_build_flags) BK_HIP(ctx, hipHostMalloc((void **)&ctx->h_build_flags, 2 * kNumCounters * sizeof(int), hipHostMallocDefault));
    return BK_OK;
}

/* launch() a pass that may flag entries, read back its counters (pinned: a pageable destination goes through the runtime's staging
 * buffer) and its flag list, again while the list overflows; the counters are cleared before each launch, the first only if `reset` */
template <typename Launch>
static int flagged_pass(bk_ctx *ctx, const char *what, BkBuildParams &bp, bool reset, Launch launch, int counters[kNumCounters],
                        std::vector<uint32_t> *flagged, int *retries = nullptr)
{
    unsigned int count = 0;
    for (;; reset = true) {
        if (reset) BK_HIP(ctx, hipMemsetAsync(ctx->d_display, 0, kNumCounters * sizeof(int), ctx->stream));
        if (hipError_t e = launch()) return ctx->fail(BK_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
        BK_HIP(ctx, hipMemcpyAsync(ctx->h_build_flags, ctx->d_display, kNumCounters * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(counters, ctx->h_build_flags, kNumCounters * sizeof(int));
        count = (unsigned)counters[BK_MAX_PLATES + 1];
        if (count <= ctx->flag_cap) break;
        (void)hipFree(ctx->d_flag_list);
        ctx->d_flag_list = nullptr;
        ctx->flag_cap = 0;
        const size_t cap = (size_t)count + count / 4 + 1024;
        BK_HIP(ctx, hipMalloc((void **)&ctx->d_flag_list, cap * 4 * sizeof(uint32_t)));
        ctx->flag_cap = cap;
        bp.flag_list = ctx->d_flag_list;                   // (nothing else in bp depends on the list)
        bp.flag_cap = (unsigned)cap;
        if (retries) ++*retries;
    }
    flagged->assign((size_t)count * 4, 0u);
    if (!count) return BK_OK;
    BK_HIP(ctx, hipMemcpyAsync(flagged->data(), ctx->d_flag_list, (size_t)count * 16, hipMemcpyDeviceToHost, ctx->stream));
    BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // The kernels append wave by wave: runs of up to 64 ascending ids.  A short list is put into the reference's scan order outright;
    // a long one (eckert4 flags whole rows: 640 K entries) is left in its runs - sorting it cost more than the re-derivation, and a
    // script's per-row cache is as warm within a run as within the sorted list.
    if (count <= 131072) sort_flagged(*flagged);
    return BK_OK;
}

/* re-derive n entries (entry i is ids[i * stride]) by the compiled host module of `source` if fixup_module gives one, else by the
 * interpreter; n == 0 or no source looks nothing up.  timed: accounted in last_host_eval_ms / last_fixup_compiled */
template <typename ModuleCall, typename InterpCall>
static void rederive(bk_ctx *ctx, LensProgram *P, const std::string &source, const uint32_t *ids, int stride, size_t n, bool timed,
                     ModuleCall module, InterpCall interp)
{
    const auto t0 = std::chrono::steady_clock::now();
    const HostModuleP hm = n && !source.empty() ? fixup_module(P, source) : nullptr;
    if (timed) ctx->last_fixup_compiled = hm != nullptr;
    if (hm) hostmod_runs(n, [&](size_t i0, size_t cnt) { module(*hm, ids + i0 * stride, stride, (unsigned long)cnt, i0); });
    else for_each_flagged(P, n, [&](HostEval &E, size_t i) { interp(E, ids[i * stride], i); });
    if (timed) ctx->last_host_eval_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

/* scatter the re-derived entries that differ from the device's answer (flag record: id, W words, a byte) to words[W * id + j] and
 * bytes[id]; counted in last_flagged / last_changed */
template <size_t W>
static int patch_changed(bk_ctx *ctx, const std::vector<uint32_t> &flagged, const uint32_t *const (&host_words)[W], const uint8_t *host_bytes,
                         uint32_t *words, uint8_t *bytes)
{
    std::vector<uint32_t> iw, vw, ib;
    std::vector<uint8_t> vb;
    const size_t nfl = flagged.size() / 4;
    for (size_t i = 0; i < nfl; ++i) {
        const uint32_t *rec = &flagged[4 * i];
        bool same = host_bytes[i] == (uint8_t)rec[1 + W];
        for (size_t j = 0; j < W; ++j) same = same && host_words[j][i] == rec[1 + j];
        if (same) continue;
        for (size_t j = 0; j < W; ++j) { iw.push_back((uint32_t)W * rec[0] + (uint32_t)j); vw.push_back(host_words[j][i]); }
        ib.push_back(rec[0]); vb.push_back(host_bytes[i]);
    }
    ctx->last_flagged = (int)nfl;
    ctx->last_changed = (int)ib.size();
    if (int r = bk::launch_scatter32(ctx, words, iw.data(), vw.data(), iw.size())) return r;
    return bk::launch_scatter8(ctx, bytes, ib.data(), vb.data(), ib.size());
}

/* Where a host-built table goes: into the context's device lensmap - or, for bk_debug_host_build on a context without a device, into the
 * caller's arrays (ctx->host_sink_*).  `off` == nullptr: the empty table.  `sub` == nullptr: every entry at its texel's centre (a forward
 * build, the empty table); it goes wherever a sub-texel plane is kept (bk_set_subtexel, bk_debug_host_build_subtexel). */
static int deliver_host_table(bk_ctx *ctx, const uint32_t *off, const uint8_t *tint, const uint16_t *sub)
{
    const size_t px = (size_t)ctx->W * ctx->rows();
    if (ctx->host_sink_off) {
        if (off) { memcpy(ctx->host_sink_off, off, px * 4); memcpy(ctx->host_sink_tint, tint, px); }
        else { memset(ctx->host_sink_off, 0xFF, px * 4); memset(ctx->host_sink_tint, 255, px); }
        if (ctx->host_sink_sub) {
            if (off && sub) memcpy(ctx->host_sink_sub, sub, px * 2);
            else memset(ctx->host_sink_sub, 0x80, px * 2);
        }
        return BK_OK;
    }
    if (off) {
        BK_HIP(ctx, hipMemcpyAsync(ctx->d_offsets, off, px * 4, hipMemcpyHostToDevice, ctx->stream));
        BK_HIP(ctx, hipMemcpyAsync(ctx->d_tints, tint, px, hipMemcpyHostToDevice, ctx->stream));
    } else {
        BK_HIP(ctx, hipMemsetAsync(ctx->d_offsets, 0xFF, px * 4, ctx->stream));
        BK_HIP(ctx, hipMemsetAsync(ctx->d_tints, 255, px, ctx->stream));
    }
    if (ctx->d_subtexel) {
        if (off && sub) BK_HIP(ctx, hipMemcpyAsync(ctx->d_subtexel, sub, px * 2, hipMemcpyHostToDevice, ctx->stream));
        else BK_HIP(ctx, hipMemsetAsync(ctx->d_subtexel, 0x80, px * 2, ctx->stream));
    }
    BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BK_OK;
}

// The inverse build as ONE sequential scan on the host (bk_set_sequential_build): what the reference does (fisheye.c:2084-2124) -
// one evaluator whose script globals travel from pixel to pixel, rows from the bottom up, pixels left to right, stopping at the
// first malformed result - by the compiled host module on the platform libm (waited for), else by the script interpreter.  For
// scripts that accumulate state across pixels, which the parallel GPU build cannot reproduce.  A stripe context scans its own rows
// with a fresh state: use a single full-height context for such scripts.
static int build_sequential(bk_ctx *ctx, LensProgram *P, const std::string &source, const BkBuildParams &bp, int display_out[BK_MAX_PLATES])
{
    const size_t px = (size_t)ctx->W * ctx->rows();
    std::vector<uint32_t> off(px, BK_NULL_OFFSET);
    std::vector<uint8_t> tint(px, 255);
    std::vector<uint16_t> sub(px, (uint16_t)0x8080);
    int disp[BK_MAX_PLATES] = {0, 0, 0, 0, 0, 0};
    int errbits = 0;
    const auto t0 = std::chrono::steady_clock::now();
    // (no generated source - the emitter declined the script, build_on_host - means no compiled host module either: the interpreter scans)
    HostModuleP hm = !source.empty() && P->interp.math == &math_platform() && bk::g_debug.host_module != 2 ? host_module_for(source, true) : nullptr;
    ctx->last_fixup_compiled = hm != nullptr;
    try {
        if (hm) errbits = hm->inverse_scan(&bp, off.data(), tint.data(), sub.data(), disp);
        else {
            const Values roots_in{P->lens_inverse, P->lens_forward, P->globe_plate};
            Values roots;
            std::unique_ptr<Interp> mine = P->interp.clone(roots_in, &roots);
            HostEval ev{mine.get(), roots[0], roots[1], roots[2]};
            for (int lyl = ctx->rows() - 1; lyl >= 0 && !errbits; --lyl)
                for (int lx = 0; lx < ctx->W && !errbits; ++lx) {
                    const size_t o = (size_t)lyl * ctx->W + lx;
                    int shown = -1;
                    h_inverse_entry(ev, bp, (uint32_t)o, &off[o], &tint[o], &sub[o], &shown, &errbits);
                    if (errbits) {
                        off[o] = BK_NULL_OFFSET; tint[o] = 255; sub[o] = 0x8080;
                        if (errbits == BK_ERR_RESULT) ctx->last_bad_key = (uint32_t)(((uint32_t)ctx->row0 + (uint32_t)lyl) * (uint32_t)ctx->W + ((uint32_t)ctx->W - 1u - (uint32_t)lx)) + 1u;
                    }
                    else if (shown >= 0) disp[shown] = 1;
                }
        }
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "lensmap build: %s", e.what());
    }
    ctx->last_host_eval_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->last_build_ms = ctx->last_host_eval_ms;
    ctx->last_flagged = ctx->last_changed = 0;
    if (errbits & ~BK_ERR_RESULT) {                              // a Lua runtime error: nothing is drawn (see bk_build)
        std::fill(off.begin(), off.end(), BK_NULL_OFFSET);
        std::fill(tint.begin(), tint.end(), (uint8_t)255);
        std::fill(sub.begin(), sub.end(), (uint16_t)0x8080);
        for (int &d : disp) d = 0;
    }
    if (int r = deliver_host_table(ctx, off.data(), tint.data(), sub.data())) return r;
    for (int i = 0; i < BK_MAX_PLATES; ++i) { ctx->display[i] = i < ctx->numplates ? disp[i] : 0; if (display_out) display_out[i] = ctx->display[i]; }
    if (errbits) return ctx->fail(BK_E_SCRIPT, "lensmap build: %s", err_text(errbits));
    return BK_OK;
}

// ---- the HOST build: scripts whose callbacks the emitter declines ---------------------------------------------------------------
// The reference lua_calls whatever the script defines (fisheye.c:1551, 1597, 1640).  The emitter turns most of Lua into GPU code,
// not all of it: recursion, tables made at run time, functions as values, strings.  Such a script is not refused: its callbacks are
// evaluated by the product's own interpreter (the evaluator calc_zoom, the globe loader and the flagged-pixel fix-up use) - on the
// worker pool, every worker on its own copy of the script state, when the callbacks provably carry nothing from one call to the
// next (bk_lens_carries_state = 0), else as ONE scan in the reference's order.  Slower by orders of magnitude than the kernels
// (seconds at 4K), and the reference's result.  Nothing here is a CPU fallback of the GPU work: the table it builds is uploaded and
// applied by the same kernels; what runs on the host is the user's Lua, which only an interpreter can run.

/* set_lensmap_from_plate (fisheye.c:1963-1982) on host tables, stripe-filtered like the kernels' commit; the tint of an on-grid
 * writer leaves an earlier off-grid writer's tint in place (set_lensmap_grid only ever sets it: 1957-1958) */
namespace {
struct HostTable { const BkBuildParams *bp; uint32_t *off; uint8_t *tint; int *disp; };
inline void h_fwd_set(const HostTable &T, int lx, int ly, int px, int py, int plate, bool offgrid)
{
    const BkBuildParams &P = *T.bp;
    if (lx < 0 || lx >= P.W || ly < 0 || ly >= P.H) return;
    T.disp[plate] = 1;                                         /* display is global, not per stripe (bk_fwd_set) */
    if (ly < P.row0 || ly >= P.row0 + P.rows) return;
    const size_t o = (size_t)(ly - P.row0) * P.W + lx;
    T.off[o] = bk_texel_offset((unsigned)P.gp, (unsigned)P.ph, (unsigned)plate, (unsigned)px, (unsigned)py);
    if (offgrid) T.tint[o] = (uint8_t)plate;
}
inline int h_wrap_sub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
/* draw_quad (fisheye.c:2246-2338) with the x86-64 build's wrap-around on INT_MIN corners; the loops visit the visible part of a
 * 2^31-long range only - the host twin of bk_draw_quad (bk_build_kernels.h), which says why that is bit-identical */
void h_draw_quad(const HostTable &T, const int *tl, const int *tr, const int *bl, const int *br, int plate, int px, int py, bool offgrid)
{
    const BkBuildParams &P = *T.bp;
    const int *p[4] = {tl, tr, br, bl};
    int x = tl[0], y = tl[1];
    int miny = y, maxy = y, minx = x, maxx = x;
    for (int i = 1; i < 4; i++) {
        const int tx = p[i][0], ty = p[i][1];
        if (tx < minx) minx = tx; else if (tx > maxx) maxx = tx;
        if (ty < miny) miny = ty; else if (ty > maxy) maxy = ty;
    }
    const int maxdiff = 20;
    {
        const int dx = h_wrap_sub(minx, maxx), dy = h_wrap_sub(miny, maxy);
        const int adx = dx < 0 ? h_wrap_sub(0, dx) : dx, ady = dy < 0 ? h_wrap_sub(0, dy) : dy;
        if (adx > maxdiff || ady > maxdiff) return;                                       /* :2272 */
    }
    const int vx0 = minx < 0 ? 0 : minx, vx1 = maxx >= P.W ? P.W - 1 : maxx;
    const int vy0 = miny < 0 ? 0 : miny, vy1 = maxy >= P.H ? P.H - 1 : maxy;
    if (miny == maxy && minx == maxx) { h_fwd_set(T, x, y, px, py, plate, offgrid); return; }
    if (miny == maxy) { for (int tx = vx0; tx <= vx1; ++tx) h_fwd_set(T, tx, miny, px, py, plate, offgrid); return; }
    if (minx == maxx) { for (int ty = vy0; ty <= vy1; ++ty) h_fwd_set(T, x, ty, px, py, plate, offgrid); return; }
    const bool tall = h_wrap_sub(maxy, miny) < 0;
    const int y_first = tall ? vy0 : miny, nrows = h_wrap_sub(tall ? vy1 : maxy, y_first);
    for (int ky = 0; ky <= nrows; ++ky) {
        y = (int)((unsigned)y_first + (unsigned)ky);
        int tx[2] = {minx, maxx};
        int txi = 0, j = 3;
        for (int i = 0; i < 4; ++i) {
            const int ix = p[i][0], iy = p[i][1], jx = p[j][0], jy = p[j][1];
            if ((iy < y && y <= jy) || (jy < y && y <= iy)) {                             /* :2310 */
                const double dy = (double)h_wrap_sub(jy, iy), dx = (double)h_wrap_sub(jx, ix);
                tx[txi] = h_trunc_to_int((double)ix + (double)h_wrap_sub(y, iy) / dy * dx); /* :2313 */
                if (++txi == 2) break;
            }
            j = i;
        }
        if (tx[0] > tx[1]) { const int t = tx[0]; tx[0] = tx[1]; tx[1] = t; }
        if (h_wrap_sub(tx[1], tx[0]) > maxdiff) return;                                   /* :2327 aborts the quad */
        const int x_first = tx[0] < 0 ? 0 : tx[0], x_last = tx[1] >= P.W ? P.W - 1 : tx[1];
        for (x = x_first; x <= x_last; ++x) h_fwd_set(T, x, y, px, py, plate, offgrid);
    }
}
}  // namespace

/* what a host build leaves in the context: the table on the device, display flags, timings, and how it was built */
static int finish_host_build(bk_ctx *ctx, const std::vector<uint32_t> &off, const std::vector<uint8_t> &tint, const uint16_t *sub /* null: all centre */,
                             const int disp[BK_MAX_PLATES], int display_out[BK_MAX_PLATES], std::chrono::steady_clock::time_point t0)
{
    ctx->last_host_eval_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->last_build_ms = ctx->last_host_eval_ms;
    ctx->last_flagged = ctx->last_changed = 0;
    if (int r = deliver_host_table(ctx, off.data(), tint.data(), sub)) return r;
    for (int i = 0; i < BK_MAX_PLATES; ++i) { ctx->display[i] = i < ctx->numplates ? disp[i] : 0; if (display_out) display_out[i] = ctx->display[i]; }
    return BK_OK;
}
static int empty_host_build(bk_ctx *ctx, int display_out[BK_MAX_PLATES], const char *what)
{
    // a Lua run-time error, which the reference's unprotected lua_call does not survive: nothing is drawn (see bk_build)
    if (int r = deliver_host_table(ctx, nullptr, nullptr, nullptr)) return r;
    for (int i = 0; i < BK_MAX_PLATES; ++i) { ctx->display[i] = 0; if (display_out) display_out[i] = 0; }
    return ctx->fail(BK_E_SCRIPT, "lensmap build: %s", what);
}

/* resume_lensmap_inverse (fisheye.c:2084-2124) on the worker pool: every pixel by the interpreter, every worker on its own copy of
 * the script state; a malformed result ends the reference's scan there, so what lies behind it in scan order is taken away again
 * (the kernels' rule: launch_truncate_scan) */
static int build_inverse_pool(bk_ctx *ctx, LensProgram *P, const BkBuildParams &bp, int display_out[BK_MAX_PLATES])
{
    const size_t px = (size_t)ctx->W * ctx->rows();
    std::vector<uint32_t> off(px, BK_NULL_OFFSET);
    std::vector<uint8_t> tint(px, 255);
    std::vector<uint16_t> sub(px, (uint16_t)0x8080);
    std::vector<int8_t> shown(px, (int8_t)-1);
    std::vector<uint8_t> err(px, 0);
    int disp[BK_MAX_PLATES] = {0, 0, 0, 0, 0, 0};
    const auto t0 = std::chrono::steady_clock::now();
    try {
        for_each_flagged(P, px, [&](HostEval &E, size_t o) {
            int s = -1, e = 0;
            h_inverse_entry(E, bp, (uint32_t)o, &off[o], &tint[o], &sub[o], &s, &e);
            shown[o] = (int8_t)s; err[o] = (uint8_t)e;
        });
    } catch (const LuaError &e) {
        return empty_host_build(ctx, display_out, e.what());
    }
    uint32_t bad_key = 0;
    for (size_t o = 0; o < px; ++o) {
        if (!err[o]) continue;
        if (err[o] & ~BK_ERR_RESULT) return empty_host_build(ctx, display_out, err_text(err[o]));
        const uint32_t lyl = (uint32_t)(o / (size_t)ctx->W), lx = (uint32_t)(o - (size_t)lyl * ctx->W);
        bad_key = std::max(bad_key, (uint32_t)(((uint32_t)ctx->row0 + lyl) * (uint32_t)ctx->W + ((uint32_t)ctx->W - 1u - lx)) + 1u);
    }
    if (bad_key) {
        // the scan reaches pixel (ly, lx) before the failing one iff its key is larger: everything else - the failing pixel too - is NULL
        for (size_t o = 0; o < px; ++o) {
            const uint32_t lyl = (uint32_t)(o / (size_t)ctx->W), lx = (uint32_t)(o - (size_t)lyl * ctx->W);
            const uint32_t key = (uint32_t)(((uint32_t)ctx->row0 + lyl) * (uint32_t)ctx->W + ((uint32_t)ctx->W - 1u - lx)) + 1u;
            if (key <= bad_key) { off[o] = BK_NULL_OFFSET; tint[o] = 255; sub[o] = 0x8080; shown[o] = -1; }
        }
    }
    for (size_t o = 0; o < px; ++o) if (shown[o] >= 0) disp[shown[o]] = 1;
    ctx->last_bad_key = bad_key;
    if (int r = finish_host_build(ctx, off, tint, sub.data(), disp, display_out, t0)) return r;
    if (bad_key) return ctx->fail(BK_E_SCRIPT, "lensmap build: %s", err_text(BK_ERR_RESULT));
    return BK_OK;
}

/* resume_lensmap_forward (fisheye.c:2126-2217) on the host.  sequential: ONE evaluator and the reference's own call order - per
 * plate the bottom row of corners, then per texel row (from the last up) its upper corners left to right and its texels' "own
 * plate" tests (globe_plate) left to right - so that state a script carries from call to call travels as in the reference.
 * Otherwise a plate's corners (and its own-plate tests, with a globe_plate script) are evaluated on the worker pool and the
 * quads are drawn afterwards in the reference's order (later writers overwrite).  A nil corner skips the quads that touch it
 * (the reference reads a stale entry there; no shipped lens returns nil: DESIGN.md 5); a malformed
 * result leaves an EMPTY lensmap, as the kernels' forward build does (blinky_hip.h). */
static int build_forward_host(bk_ctx *ctx, LensProgram *P, const BkBuildParams &bp, bool sequential, int display_out[BK_MAX_PLATES])
{
    const size_t px_total = (size_t)ctx->W * ctx->rows();
    std::vector<uint32_t> off(px_total, BK_NULL_OFFSET);
    std::vector<uint8_t> tint(px_total, 255);
    int disp[BK_MAX_PLATES] = {0, 0, 0, 0, 0, 0};
    const HostTable T{&bp, off.data(), tint.data(), disp};
    const int ps = bp.ps, n1 = ps + 1;
    const size_t ncorner = (size_t)n1 * n1;
    std::vector<int> cx(ncorner), cy(ncorner), cerr(ncorner);
    std::vector<uint8_t> cok(ncorner), own((size_t)ps * ps, 1);
    const auto t0 = std::chrono::steady_clock::now();
    int errbits = 0;
    auto draw_row = [&](int plate, int py) {
        for (int px = 0; px < ps; ++px) {
            if (!own[(size_t)py * ps + px]) continue;                                               /* :2196 */
            const size_t c_tl = (size_t)py * n1 + px, c_bl = c_tl + n1;
            if (!(cok[c_tl] && cok[c_tl + 1] && cok[c_bl] && cok[c_bl + 1])) continue;
            const int tl[2] = {cx[c_tl], cy[c_tl]}, tr[2] = {cx[c_tl + 1], cy[c_tl + 1]}, bl[2] = {cx[c_bl], cy[c_bl]}, br[2] = {cx[c_bl + 1], cy[c_bl + 1]};
            h_draw_quad(T, tl, tr, bl, br, plate, px, py, h_offgrid(bp, px, py));
        }
    };
    try {
        const Values roots_in{P->lens_inverse, P->lens_forward, P->globe_plate};
        Values roots;
        std::unique_ptr<Interp> mine = P->interp.clone(roots_in, &roots);
        HostEval ev{mine.get(), roots[0], roots[1], roots[2]};
        for (int plate = 0; plate < bp.numplates && !errbits; ++plate) {
            const uint32_t c0 = (uint32_t)((size_t)plate * ncorner), t0id = (uint32_t)((size_t)plate * ps * ps);
            if (sequential) {
                auto corner_row = [&](int j) {
                    for (int i = 0; i < n1 && !errbits; ++i) {
                        const size_t k = (size_t)j * n1 + i;
                        h_corner_entry(ctx, ev, bp, c0 + (uint32_t)k, &cx[k], &cy[k], &cok[k], &errbits);
                    }
                };
                corner_row(ps);                                                                  /* :2148 the lower points of the last row */
                for (int py = ps - 1; py >= 0 && !errbits; --py) {
                    corner_row(py);                                                              /* :2172 upper points */
                    if (errbits) break;
                    for (int px = 0; px < ps; ++px) own[(size_t)py * ps + px] = h_texel_owns(ctx, ev, bp, t0id + (uint32_t)((size_t)py * ps + px)) ? 1 : 0;
                    draw_row(plate, py);
                }
            } else {
                std::fill(cerr.begin(), cerr.end(), 0);
                for_each_flagged(P, ncorner, [&](HostEval &E, size_t k) { h_corner_entry(ctx, E, bp, c0 + (uint32_t)k, &cx[k], &cy[k], &cok[k], &cerr[k]); });
                for (size_t k = 0; k < ncorner; ++k) errbits |= cerr[k];
                if (errbits) break;
                if (bp.has_globe_plate) for_each_flagged(P, (size_t)ps * ps, [&](HostEval &E, size_t k) { own[k] = h_texel_owns(ctx, E, bp, t0id + (uint32_t)k) ? 1 : 0; });
                else for (size_t k = 0; k < (size_t)ps * ps; ++k) own[k] = h_texel_owns(ctx, ev, bp, t0id + (uint32_t)k) ? 1 : 0;
                for (int py = ps - 1; py >= 0; --py) draw_row(plate, py);
            }
        }
    } catch (const LuaError &e) {
        return empty_host_build(ctx, display_out, e.what());
    }
    if (errbits) return empty_host_build(ctx, display_out, err_text(errbits));
    return finish_host_build(ctx, off, tint, nullptr, disp, display_out, t0);      // (the quad rasteriser has no per-pixel uv: every entry at its texel's centre)
}

/* bk_build for a script the emitter declined (`why` = its refusal) */
static int build_on_host(bk_ctx *ctx, LensProgram *P, const std::string &why, int display_out[BK_MAX_PLATES])
{
    BkBuildParams bp;
    fill_params(ctx, &bp);
    bk::EmitRequest rq;
    rq.interp = &P->interp; rq.lens_inverse = P->lens_inverse; rq.lens_forward = P->lens_forward; rq.globe_plate = P->globe_plate;
    std::string which;
    bool carries = true;                                   // (a script the state analysis cannot follow either is taken to carry state)
    try { carries = bk::callbacks_carry_state(rq, &which); } catch (const LuaError &) { carries = true; which = "(callbacks not analysable)"; }
    const bool sequential = ctx->sequential_build >= 2 || (ctx->sequential_build == 1 && carries);
    ctx->last_build_path = sequential ? 2 : 1;
    ctx->last_build_why = why + (sequential ? (carries ? "; state carried in '" + which + "': one sequential scan on the host" : "; one sequential scan on the host (bk_set_sequential_build 2)")
                                            : "; callbacks carry no state: evaluated on the host's worker pool");
    if (P->info.map_type == BK_MAP_INVERSE) {
        if (!P->lens_inverse.is_function()) return ctx->fail(BK_E_STATE, "lens has no lens_inverse (map = \"lens_inverse\" without the function)");
        return sequential ? build_sequential(ctx, P, std::string(), bp, display_out) : build_inverse_pool(ctx, P, bp, display_out);
    }
    if (!P->lens_forward.is_function()) return ctx->fail(BK_E_STATE, "lens has no lens_forward");
    return build_forward_host(ctx, P, bp, sequential, display_out);
}

/* how the last bk_build evaluated the lens callbacks: 0 = the GPU kernels, 1 = the host's worker pool, 2 = one sequential scan on the
 * host; `why` (nullable) receives the reason for 1 / 2 - the construct the emitter declined, and the state finding */
extern "C" int bk_last_build_path(const bk_ctx *ctx, char *why, size_t cap)
{
    if (!ctx) return BK_E_INVALID;
    if (why && cap) snprintf(why, cap, "%s", ctx->last_build_why.c_str());
    return ctx->last_build_path;
}

#if BK_DEBUG_API
/* test hook: the HOST build paths on any context, a device-less one included (the CPU suite and the sanitizer run reach them this way).
 * mode 1 = the worker pool, 2 = one sequential scan, 0 = whichever bk_build would take for a script the emitter declines.  The table
 * comes back in the reference's layout (plate * ps * ps + py * ps + px, 0xFFFFFFFF = NULL); display_out as bk_build's; the return value
 * is bk_build's (BK_E_SCRIPT with the truncated / empty table in place).  Inverse maps never use the compiled host module here. */
static int debug_host_build(bk_ctx *ctx, int mode, uint32_t *offsets, uint8_t *tints, uint16_t *sub /* nullable */, int display_out[BK_MAX_PLATES],
                            double *scale_out)
{
    if (!ctx || !offsets || !tints || mode < 0 || mode > 2) return BK_E_INVALID;
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid) return ctx->fail(BK_E_STATE, "not a valid lens");
    if (!ctx->globe_valid) return ctx->fail(BK_E_STATE, "not a valid globe");
    if (ctx->W <= 0 || ctx->rows() <= 0) return ctx->fail(BK_E_STATE, "bk_debug_host_build: call bk_resize first");
    const size_t px = (size_t)ctx->W * ctx->rows();
    memset(offsets, 0xFF, px * 4);
    memset(tints, 255, px);
    if (sub) memset(sub, 0x80, px * 2);
    for (int i = 0; i < BK_MAX_PLATES; ++i) { ctx->display[i] = 0; if (display_out) display_out[i] = 0; }
    ctx->last_bad_key = 0;
    if (int r = bk_calc_zoom(ctx, scale_out)) return r;
    if (P->info.map_type == BK_MAP_NONE) return ctx->fail(BK_E_STATE, "no inverse or forward map being used");
    BkBuildParams bp;
    fill_params(ctx, &bp);
    ctx->host_sink_off = offsets; ctx->host_sink_tint = tints; ctx->host_sink_sub = sub;
    int rc;
    if (mode == 0) rc = build_on_host(ctx, P, "bk_debug_host_build", display_out);
    else if (P->info.map_type == BK_MAP_INVERSE) {
        if (!P->lens_inverse.is_function()) rc = ctx->fail(BK_E_STATE, "lens has no lens_inverse");
        else rc = mode == 2 ? build_sequential(ctx, P, std::string(), bp, display_out) : build_inverse_pool(ctx, P, bp, display_out);
    } else {
        if (!P->lens_forward.is_function()) rc = ctx->fail(BK_E_STATE, "lens has no lens_forward");
        else rc = build_forward_host(ctx, P, bp, mode == 2, display_out);
    }
    ctx->host_sink_off = nullptr; ctx->host_sink_tint = nullptr; ctx->host_sink_sub = nullptr;
    for (size_t i = 0; i < px; ++i) {
        if (offsets[i] == BK_NULL_OFFSET) continue;
        unsigned plate, x, y;
        bk_texel_coords((unsigned)ctx->gp, (unsigned)ctx->ph, offsets[i], &plate, &x, &y);
        offsets[i] = plate * (unsigned)(ctx->ps * ctx->ps) + y * (unsigned)ctx->ps + x;
    }
    return rc;
}
extern "C" int bk_debug_host_build(bk_ctx *ctx, int mode, uint32_t *offsets, uint8_t *tints, int display_out[BK_MAX_PLATES], double *scale_out)
{
    return debug_host_build(ctx, mode, offsets, tints, nullptr, display_out, scale_out);
}
/* ... with the sub-texel plane the same build keeps under bk_set_subtexel (uint16 [rows][W]: qx | qy << 8, 0x8080 where the entry has no
 * position of its own - NULL entries, every entry of a forward map); the context's switch plays no part */
extern "C" int bk_debug_host_build_subtexel(bk_ctx *ctx, int mode, uint32_t *offsets, uint8_t *tints, uint16_t *sub, int display_out[BK_MAX_PLATES],
                                            double *scale_out)
{
    if (!sub) return BK_E_INVALID;
    return debug_host_build(ctx, mode, offsets, tints, sub, display_out, scale_out);
}
#endif

extern "C" int bk_set_sequential_build(bk_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return BK_E_INVALID;
    ctx->sequential_build = mode;
    return BK_OK;
}

/* 1 if a callback of the current lens / globe reads a script global that callbacks assign before assigning it itself (state can
 * travel from pixel to pixel), 0 if not, negative on error; `global_name` (nullable) receives the first such global */
extern "C" int bk_lens_carries_state(bk_ctx *ctx, char *global_name, size_t cap)
{
    if (!ctx) return BK_E_INVALID;
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid) return ctx->fail(BK_E_STATE, "not a valid lens");
    bk::EmitRequest rq;
    rq.interp = &P->interp; rq.lens_inverse = P->lens_inverse; rq.lens_forward = P->lens_forward; rq.globe_plate = P->globe_plate;
    std::string which;
    bool carries = false;
    try { carries = bk::callbacks_carry_state(rq, &which); } catch (const LuaError &e) { return ctx->fail(BK_E_SCRIPT, "%s", e.what()); }
    if (global_name && cap) snprintf(global_name, cap, "%s", which.c_str());
    return carries ? 1 : 0;
}

struct HipFree { void operator()(void *p) const { (void)hipFree(p); } };
using DeviceMem = std::unique_ptr<void, HipFree>;

/* the inverse build on the device; counters: the pass's, with the re-derived entries' display flags, errors and first bad key merged in */
static int build_inverse_device(bk_ctx *ctx, LensProgram *P, const std::string &src, BkBuildParams &bp, int counters[kNumCounters])
{
    if (!P->k_inverse) return ctx->fail(BK_E_STATE, "lens has no lens_inverse (map = \"lens_inverse\" without the function)");
    for (int k = 0; k < 4; ++k) {                     // (a forward build's scratch is not kept under an inverse lens)
        (void)hipFree(ctx->fwd_scratch[k]);
        ctx->fwd_scratch[k] = nullptr; ctx->fwd_scratch_bytes[k] = 0;
    }
    void *args[] = {&bp};
    BK_HIP(ctx, hipEventRecord(ctx->build_time_ev[0], ctx->stream));
    const auto tk0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> flagged;
    if (int r = flagged_pass(ctx, "bk_build_inverse launch", bp, false, [&] {
            return hipModuleLaunchKernel(P->k_inverse, (unsigned)((ctx->W + 255) / 256), (unsigned)ctx->rows(), 1, 256, 1, 1, 0, ctx->stream, args, nullptr);
        }, counters, &flagged, &ctx->last_kernel_retries)) return r;
    ctx->last_kernel_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tk0).count();
    // re-derive the flagged pixels on the host and patch the ones that differ
    const size_t nfl = flagged.size() / 4;
    std::vector<uint32_t> roff(nfl);
    std::vector<uint8_t> rtint(nfl);
    std::vector<uint16_t> rsub(nfl);
    std::vector<int> rshown(nfl), rerr(nfl, 0);
    rederive(ctx, P, src, flagged.data(), 4, nfl, true,
             [&](const HostModule &hm, const uint32_t *id, int stride, unsigned long cnt, size_t i) { hm.inverse(&bp, id, stride, cnt, &roff[i], &rtint[i], &rsub[i], &rshown[i], &rerr[i]); },
             [&](HostEval &E, uint32_t id, size_t i) { h_inverse_entry(E, bp, id, &roff[i], &rtint[i], &rsub[i], &rshown[i], &rerr[i]); });
    unsigned int bad_key = (unsigned)counters[BK_MAX_PLATES + 2];
    for (size_t i = 0; i < nfl; ++i) {
        counters[BK_MAX_PLATES] |= rerr[i];
        if (rerr[i] & BK_ERR_RESULT) {
            const uint32_t o = flagged[4 * i], lyl = o / (uint32_t)ctx->W, lx = o - lyl * (uint32_t)ctx->W;
            bad_key = std::max(bad_key, (uint32_t)(((uint32_t)ctx->row0 + lyl) * (uint32_t)ctx->W + ((uint32_t)ctx->W - 1u - lx)) + 1u);
        }
        if (rshown[i] >= 0) counters[rshown[i]] |= 1;
    }
    counters[BK_MAX_PLATES + 2] = (int)bad_key;
    if (int r = patch_changed(ctx, flagged, {roff.data()}, rtint.data(), ctx->d_offsets, ctx->d_tints)) return r;
    // the sub-texel plane of the flagged entries: a ray component narrowed to the neighbouring float moves u by an ulp - the offset may
    // stay and the sub still differ - so it is compared and patched on its own (the record's fourth word is the device's); last_changed
    // keeps counting offsets and tints only
    if (bp.subtexel) {
        std::vector<uint32_t> is;
        std::vector<uint16_t> vs;
        for (size_t i = 0; i < nfl; ++i)
            if (rsub[i] != (uint16_t)flagged[4 * i + 3]) { is.push_back(flagged[4 * i]); vs.push_back(rsub[i]); }
        if (int r = bk::launch_scatter16(ctx, bp.subtexel, is.data(), vs.data(), is.size())) return r;
    }
    BK_HIP(ctx, hipEventRecord(ctx->build_time_ev[1], ctx->stream));
    return BK_OK;
}

/* the forward build on the device; counters: the quad pass's, with the corner pass's and the host's error bits merged in */
static int build_forward_device(bk_ctx *ctx, LensProgram *P, const std::string &src, BkBuildParams &bp, int counters[kNumCounters])
{
    if (!P->k_corners || !P->k_quads || !P->k_resolve) return ctx->fail(BK_E_STATE, "lens has no lens_forward");
    const size_t px = (size_t)ctx->W * ctx->rows();
    const size_t n1 = (size_t)ctx->ps + 1;
    const size_t ncorner = (size_t)ctx->numplates * n1 * n1;
    // bk_debug_set_forward_corners: the test's table goes where the corner pass would have put its own
    const bool given = ctx->debug_corners_set();
    (void)given;
#if BK_DEBUG_API
    if (given && ctx->dbg_corner_ok.size() != ncorner)
        return ctx->fail(BK_E_INVALID, "bk_debug_set_forward_corners: the table has %zu corners, this build has %zu (plates * (platesize + 1)^2)", ctx->dbg_corner_ok.size(), ncorner);
#endif
    const size_t want[4] = {ncorner * 2 * sizeof(int), ncorner, px * 4, px * 4};
    for (int k = 0; k < 4; ++k)
        if (ctx->fwd_scratch_bytes[k] < want[k]) {
            (void)hipFree(ctx->fwd_scratch[k]);
            ctx->fwd_scratch[k] = nullptr; ctx->fwd_scratch_bytes[k] = 0;
            BK_HIP(ctx, hipMalloc(&ctx->fwd_scratch[k], want[k]));
            ctx->fwd_scratch_bytes[k] = want[k];
        }
    bp.corner_xy = (int *)ctx->fwd_scratch[0];
    bp.corner_ok = (unsigned char *)ctx->fwd_scratch[1];
    bp.fwd_key_px = (unsigned int *)ctx->fwd_scratch[2];
    bp.fwd_key_tint = (unsigned int *)ctx->fwd_scratch[3];
    // the quotient / uv tables of bk_build_params.h: plain IEEE divisions, done here once per platesize instead of per texel
    constexpr size_t NQ = 21 * 21;
    const size_t ntile = ((size_t)ctx->ps + 15) / 16;              // (BK_FWD_TILE = 16; the tile flags of bk_forward_tiles live behind the tables)
    if (ctx->fwd_tables_ps != ctx->ps) {
        (void)hipFree(ctx->fwd_tables);
        ctx->fwd_tables = nullptr; ctx->fwd_tables_ps = -1;
        std::vector<double> q(NQ, 0.0);
        for (int a = 0; a <= 20; ++a)
            for (int d = 1; d <= 20; ++d) q[(size_t)a * 21 + d] = (double)a / (double)d;
        std::vector<float> uv(2 * n1);
        for (size_t i = 0; i < n1; ++i) {
            uv[i] = (float)(((double)i - 0.5) / ctx->ps - 0.5);
            uv[n1 + i] = (float)((double)i / ctx->ps - 0.5);
        }
        BK_HIP(ctx, hipMalloc(&ctx->fwd_tables, NQ * sizeof(double) + uv.size() * sizeof(float) + (size_t)BK_MAX_PLATES * ntile * ntile));
        BK_HIP(ctx, hipMemcpy(ctx->fwd_tables, q.data(), NQ * sizeof(double), hipMemcpyHostToDevice));
        BK_HIP(ctx, hipMemcpy((char *)ctx->fwd_tables + NQ * sizeof(double), uv.data(), uv.size() * sizeof(float), hipMemcpyHostToDevice));
        ctx->fwd_tables_ps = ctx->ps;
    }
    bp.fwd_quot = (const double *)ctx->fwd_tables;
    bp.fwd_uv = (const float *)((const char *)ctx->fwd_tables + NQ * sizeof(double));
    unsigned char *const tile_own = (unsigned char *)ctx->fwd_tables + NQ * sizeof(double) + 2 * n1 * sizeof(float);
    const hipEvent_t e0 = ctx->build_time_ev[0], e1 = ctx->build_time_ev[1];
    void *args[] = {&bp};
    const auto clear_keys = [&](hipStream_t st) -> hipError_t {
        hipError_t e = hipMemsetAsync(ctx->fwd_scratch[2], 0, px * 4, st);
        return e == hipSuccess ? hipMemsetAsync(ctx->fwd_scratch[3], 0, px * 4, st) : e;
    };
    const auto launch_corners = [&]() -> hipError_t {
#if BK_DEBUG_API
        if (given) {
            hipError_t e = hipMemcpyAsync(bp.corner_xy, ctx->dbg_corner_xy.data(), ncorner * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
            return e == hipSuccess ? hipMemcpyAsync(bp.corner_ok, ctx->dbg_corner_ok.data(), ncorner, hipMemcpyHostToDevice, ctx->stream) : e;
        }
#endif
        return hipModuleLaunchKernel(P->k_corners, (unsigned)((n1 + 255) / 256), (unsigned)n1, (unsigned)ctx->numplates, 256, 1, 1, 0, ctx->stream, args, nullptr);
    };
    const auto launch_quads = [&](bool keys_cleared = false, void **with = nullptr) -> hipError_t {
        hipError_t e = keys_cleared ? hipSuccess : clear_keys(ctx->stream);
        if (e == hipSuccess) e = hipModuleLaunchKernel(P->k_quads, (unsigned)((ctx->ps + 15) / 16), (unsigned)((ctx->ps + 15) / 16), (unsigned)ctx->numplates, 256, 1, 1, 0,
                                                       ctx->stream, with ? with : args, nullptr);       // (BK_FWD_TILE = 16: bk_build_kernels.h)
        return e;
    };
    const auto launch_resolve = [&](void **with = nullptr) -> hipError_t {
        return hipModuleLaunchKernel(P->k_resolve, (unsigned)((px + 255) / 256), 1, 1, 256, 1, 1, 0, ctx->stream, with ? with : args, nullptr);
    };
    // The three passes in one go, each of the first two counting into its own set of counters, both sets left in pinned memory
    // by the last pass: nearly every build flags nothing - no corner and no texel for the host
    // to look at again - and then the table is final when the stream drains, two stops (a read-back and a decision each, 25-30 us
    // apiece at 4K) earlier.  A build that did flag something is done over the careful way below, and so is the next build of
    // the same lens.
    if (!P->fwd_needs_host && !bk::g_debug.forward_careful) {
        int *const after_corners = ctx->h_build_flags, *const after_quads = ctx->h_build_flags + kNumCounters;
        if (!ctx->build_aux) {
            BK_HIP(ctx, hipStreamCreateWithFlags(&ctx->build_aux, hipStreamNonBlocking));
            for (hipEvent_t &e : ctx->build_ev) BK_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        BK_HIP(ctx, hipEventRecord(e0, ctx->stream));
        BK_HIP(ctx, hipEventRecord(ctx->build_ev[0], ctx->stream));
        BK_HIP(ctx, launch_corners());
        // the key planes (66 MB at 4K) are cleared on the side stream while the corner pass - arithmetic only - has the chip
        // (after whatever the stream held before this build, which may still read them: build_ev[0])
        BK_HIP(ctx, hipStreamWaitEvent(ctx->build_aux, ctx->build_ev[0], 0));
        BK_HIP(ctx, clear_keys(ctx->build_aux));
        // ... and the tiles that lie wholly inside their plate's own region are found there too (the plates may have changed
        // since the last build: 110 K threads, a few microseconds)
        BkBuildParams bq = bp;
        if (P->k_tiles) {
            unsigned char *flags_out = tile_own;
            void *args_t[] = {&bp, &flags_out};
            BK_HIP(ctx, hipModuleLaunchKernel(P->k_tiles, (unsigned)((ntile * ntile + 255) / 256), (unsigned)ctx->numplates, 1, 256, 1, 1, 0, ctx->build_aux, args_t, nullptr));
            bq.tile_own = tile_own;
            ctx->fwd_tiles_used = true;
        }
        BK_HIP(ctx, hipEventRecord(ctx->build_ev[1], ctx->build_aux));
        bq.display = ctx->d_display + kNumCounters;       // the quad pass counts into the second set (cleared with the first by bk_build)
        bq.err = bq.display + BK_MAX_PLATES;
        bq.flag_count = (unsigned int *)(bq.display + BK_MAX_PLATES + 1);
        bq.first_bad = (unsigned int *)(bq.display + BK_MAX_PLATES + 2);
        void *args_q[] = {&bq};
        BK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->build_ev[1], 0));
        BK_HIP(ctx, launch_quads(true, args_q));
        static_assert(2 * kNumCounters == 18, "bk_forward_resolve copies 18 counters");
        BkBuildParams br = bp;
        br.counters_out = ctx->h_build_flags;
        void *args_r[] = {&br};
        BK_HIP(ctx, launch_resolve(args_r));
        BK_HIP(ctx, hipEventRecord(e1, ctx->stream));
        BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (after_corners[BK_MAX_PLATES + 1] == 0 && after_quads[BK_MAX_PLATES + 1] == 0) {
            memcpy(counters, after_quads, kNumCounters * sizeof(int));
            counters[BK_MAX_PLATES] |= after_corners[BK_MAX_PLATES];
            ctx->last_flagged = 0;
            ctx->last_changed = 0;
            return BK_OK;
        }
        P->fwd_needs_host = true;
        ctx->fwd_tiles_used = false;
        BK_HIP(ctx, hipMemsetAsync(ctx->d_display, 0, kNumCounters * sizeof(int), ctx->stream));
    }
    BK_HIP(ctx, hipEventRecord(e0, ctx->stream));
    // texel corners -> screen; the flagged ones re-derived on the host
    std::vector<uint32_t> flagged;
    if (int r = flagged_pass(ctx, "bk_forward_corners launch", bp, false, launch_corners, counters, &flagged)) return r;
    const size_t nfl = flagged.size() / 4;
    std::vector<int> rsx(nfl), rsy(nfl), rerr(nfl, 0);
    std::vector<uint8_t> rok(nfl);
    rederive(ctx, P, src, flagged.data(), 4, nfl, true,
             [&](const HostModule &hm, const uint32_t *id, int stride, unsigned long cnt, size_t i) { hm.corners(&bp, id, stride, cnt, &rsx[i], &rsy[i], &rok[i], &rerr[i]); },
             [&](HostEval &E, uint32_t id, size_t i) { h_corner_entry(ctx, E, bp, id, &rsx[i], &rsy[i], &rok[i], &rerr[i]); });
    int corner_err = counters[BK_MAX_PLATES];
    for (int e : rerr) corner_err |= e;
    if (int r = patch_changed(ctx, flagged, {(const uint32_t *)rsx.data(), (const uint32_t *)rsy.data()}, rok.data(), (uint32_t *)bp.corner_xy, bp.corner_ok)) return r;
    // quads; with a globe_plate script a texel's "own plate" test can be flagged too: the host answers those, and if an answer
    // differs from the device's the pass runs once more with the host's answers in place (flagging nothing then)
    if (int r = flagged_pass(ctx, "bk_forward_quads launch", bp, true, launch_quads, counters, &flagged)) return r;
    DeviceMem d_ovr;
    if (!flagged.empty()) {
        const size_t nown = flagged.size() / 4;
        std::vector<uint8_t> rown(nown);
        rederive(ctx, P, src, flagged.data(), 4, nown, false,
                 [&](const HostModule &hm, const uint32_t *id, int stride, unsigned long cnt, size_t i) { hm.texel_owns(&bp, id, stride, cnt, &rown[i]); },
                 [&](HostEval &E, uint32_t id, size_t i) { rown[i] = h_texel_owns(ctx, E, bp, id) ? 1 : 0; });
        std::vector<uint32_t> ovr(nown);                  // texel id << 1 | the host's answer
        int changed = 0;
        for (size_t i = 0; i < nown; ++i) {
            const uint32_t own = rown[i] ? 1u : 0u;
            changed += own != flagged[4 * i + 1];
            ovr[i] = flagged[4 * i] << 1 | own;
        }
        ctx->last_flagged += (int)nown;
        ctx->last_changed += changed;
        if (changed) {
            std::sort(ovr.begin(), ovr.end());
            void *d = nullptr;
            BK_HIP(ctx, hipMalloc(&d, ovr.size() * 4));
            d_ovr.reset(d);
            BK_HIP(ctx, hipMemcpyAsync(d, ovr.data(), ovr.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            bp.ovr_list = (const unsigned int *)d;
            bp.ovr_count = (unsigned)ovr.size();
            if (int r = flagged_pass(ctx, "bk_forward_quads launch", bp, true, launch_quads, counters, &flagged)) return r;
        }
    }
    counters[BK_MAX_PLATES] |= corner_err;
    BK_HIP(ctx, launch_resolve());
    BK_HIP(ctx, hipEventRecord(e1, ctx->stream));
    P->fwd_needs_host = ctx->last_flagged != 0;
    return BK_OK;
}

extern "C" int bk_build(bk_ctx *ctx, int display_out[BK_MAX_PLATES], double *scale_out)
{
    if (!ctx) return BK_E_INVALID;
    if (ctx->device < 0) return ctx->fail(BK_E_STATE, "bk_build: this context has no device");
    if (!ctx->d_offsets) return ctx->fail(BK_E_STATE, "bk_build: call bk_resize first");
    BK_HIP(ctx, hipSetDevice(ctx->device));
    bk::resident_quiesce(ctx);
    bk::Range range("bk_build");
    LensProgram *P = ctx->prog;
    if (bk::build_module_ready(ctx) == BK_PENDING) return BK_PENDING;
    const size_t px = (size_t)ctx->W * ctx->rows();
    if (int r = bk::subtexel_alloc(ctx)) return r;    // (bk_set_subtexel: from here on the plane follows the lensmap, on every way out)
    // F_RenderView clears the maps before (re)building, fisheye.c:731-732; whatever fails below,
    // the lensmap stays valid-and-empty so that bk_apply draws nothing, as the reference does.
    // (the device passes write every entry of the owned rows, so the clearing - 41 MB at 4K - is left to the ways out that have not
    //  filled the table: `empty_unless_built`; the host paths are handed a cleared table up front, as before)
    struct EmptyUnlessBuilt {
        bk_ctx *ctx; size_t px; bool armed = true;
        void now()
        {
            if (!armed) return;
            (void)hipMemsetAsync(ctx->d_offsets, 0xFF, px * 4, ctx->stream); (void)hipMemsetAsync(ctx->d_tints, 255, px, ctx->stream);
            if (ctx->d_subtexel) (void)hipMemsetAsync(ctx->d_subtexel, 0x80, px * 2, ctx->stream);      // (0x8080: every entry at its texel's centre)
            armed = false;
        }
        ~EmptyUnlessBuilt() { now(); }
    } empty_unless_built{ctx, px};
    BK_HIP(ctx, hipMemsetAsync(ctx->d_display, 0, 2 * kNumCounters * sizeof(int), ctx->stream));      // (two sets of counters: see the forward build)
    bk::lensmap_replaced(ctx);                        // (here, in front of every way out: whatever the build leaves in the table is new)
    ctx->last_bad_key = 0;
    for (int i = 0; i < BK_MAX_PLATES; ++i) { ctx->display[i] = 0; if (display_out) display_out[i] = 0; }
    ctx->last_build_ms = 0;
    ctx->last_host_eval_ms = ctx->last_kernel_wall_ms = 0;
    ctx->last_kernel_retries = 0;
    ctx->last_fixup_compiled = false;
    ctx->last_flagged = ctx->last_changed = 0;
    ctx->last_build_path = 0;
    ctx->last_build_why.clear();
    ctx->fwd_tiles_used = false;

    if (!P || !P->lens_valid) return ctx->fail(BK_E_STATE, "not a valid lens");               /* create_lensmap :2372 */
    if (!ctx->globe_valid) return ctx->fail(BK_E_STATE, "not a valid globe");
    // Callbacks that were found to change nothing a script can see (LensProgram::emitted) leave the interpreter's activity count where
    // the translation unit was generated, however often this build runs them - calc_zoom, the flagged entries; a build runs nothing
    // else: the next bk_build of the same lens finds its translation unit still valid.
    struct KeepActivity {
        LensProgram *P; unsigned long long at; bool armed;
        ~KeepActivity() { if (P->emitted.valid && P->emitted.stateless && P->emitted.activity >= at) P->interp.activity = P->emitted.activity; }
    } keep_activity{P, P->interp.activity, P->emitted.valid && P->emitted.stateless && P->emitted.activity == P->interp.activity};
    if (int r = bk_calc_zoom(ctx, scale_out)) return r;                                        /* :2376 */
    if (P->info.map_type == BK_MAP_NONE) return ctx->fail(BK_E_STATE, "no inverse or forward map being used");   /* :2395 */

    // a table from bk_debug_set_forward_corners and a build that would never read it (a host path, an inverse map): the test that set
    // it would be looking at the lens's own map - an error instead, before any work, over the empty map `empty_unless_built` leaves
    const auto unread_table = [&] {
        return ctx->fail(BK_E_STATE, "bk_build: a corner table is set (bk_debug_set_forward_corners) and this build does not run the forward passes on the device");
    };
    std::string src, refused;
    if (keep_activity.armed) P->interp.activity = keep_activity.at;      // (calc_zoom ran the callbacks: they are stateless)
    if (int r = generate_source(ctx, P, &src, &refused)) return r;
    if (!refused.empty() && ctx->debug_corners_set()) return unread_table();
    if (!refused.empty()) { empty_unless_built.now(); return build_on_host(ctx, P, refused, display_out); }     // callbacks the emitter declines: the interpreter evaluates them
    if (int r = compile_module(ctx, P, src)) return r;
    if (int r = alloc_flag_buffers(ctx)) return r;

    BkBuildParams bp;
    fill_params(ctx, &bp);
    // bk_set_sequential_build: a lens whose callbacks carry state from pixel to pixel (or every lens, mode 2) is built the way the
    // reference builds it - one evaluator, its scan order - on the host
    if ((P->info.map_type == BK_MAP_INVERSE || P->info.map_type == BK_MAP_FORWARD) && ctx->sequential_build) {
        bk::EmitRequest rq;
        rq.interp = &P->interp; rq.lens_inverse = P->lens_inverse; rq.lens_forward = P->lens_forward; rq.globe_plate = P->globe_plate;
        std::string which;
        if (ctx->sequential_build >= 2 || bk::callbacks_carry_state(rq, &which)) {
            if (ctx->debug_corners_set()) return unread_table();
            ctx->last_build_path = 2;
            ctx->last_build_why = ctx->sequential_build >= 2 ? "bk_set_sequential_build 2" : "state carried in '" + which + "'";
            empty_unless_built.now();
            if (P->info.map_type == BK_MAP_INVERSE) return build_sequential(ctx, P, src, bp, display_out);
            // (r6) the forward scan is just as sequential in the reference (fisheye.c:2126-2217): its call order, one evaluator
            if (!P->lens_forward.is_function()) return ctx->fail(BK_E_STATE, "lens has no lens_forward");
            return build_forward_host(ctx, P, bp, true, display_out);
        }
    }
    if (P->info.map_type != BK_MAP_FORWARD && ctx->debug_corners_set()) return unread_table();
    for (hipEvent_t &e : ctx->build_time_ev) if (!e) BK_HIP(ctx, hipEventCreate(&e));
    int counters[kNumCounters];
    try {
        const bool inverse = P->info.map_type == BK_MAP_INVERSE;
        // (the forward passes know texels, not where in them a pixel's ray lands: the plane is all centres)
        if (!inverse && ctx->d_subtexel) BK_HIP(ctx, hipMemsetAsync(ctx->d_subtexel, 0x80, px * 2, ctx->stream));
        if (int r = inverse ? build_inverse_device(ctx, P, src, bp, counters) : build_forward_device(ctx, P, src, bp, counters)) return r;
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "lensmap build: %s", e.what());
    }
    BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->build_time_ev[0], ctx->build_time_ev[1]);
    ctx->last_build_ms = ms;
    for (int i = 0; i < BK_MAX_PLATES; ++i) {
        ctx->display[i] = i < ctx->numplates ? counters[i] : 0;
        if (display_out) display_out[i] = ctx->display[i];
    }
    const int errbits = counters[BK_MAX_PLATES];
    if (errbits == BK_ERR_RESULT && P->info.map_type == BK_MAP_INVERSE) {
        // A malformed callback result (status -1) ends the reference's scan at that pixel and KEEPS what it had set by then
        // (fisheye.c:2113-2117; rows from the bottom up, pixels left to right; run to completion, no time slicing).  The GPU
        // build has evaluated every pixel: take away what the reference had not reached, recount the display flags, and
        // report the error with that table in place.  (A stripe context knows only its own rows: bk_multi_build / the host
        // of a bk_comm group hands every stripe the group's first failing pixel - bk_truncate_build.)
        ctx->last_bad_key = (unsigned int)counters[BK_MAX_PLATES + 2];
        int disp[BK_MAX_PLATES];
        if (int r = bk::launch_truncate_scan(ctx, ctx->last_bad_key, disp)) return r;
        for (int i = 0; i < BK_MAX_PLATES; ++i) { ctx->display[i] = i < ctx->numplates ? disp[i] : 0; if (display_out) display_out[i] = ctx->display[i]; }
        empty_unless_built.armed = false;
        return ctx->fail(BK_E_SCRIPT, "lensmap build: %s", err_text(errbits));
    }
    if (errbits) {
        // Any other per-pixel error is a Lua runtime error, which the reference does not survive (lua_call is unprotected:
        // fisheye.c:1551); here the build leaves an EMPTY map (nothing is drawn) and reports it.
        empty_unless_built.now();
        BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < BK_MAX_PLATES; ++i) { ctx->display[i] = 0; if (display_out) display_out[i] = 0; }
        return ctx->fail(BK_E_SCRIPT, "lensmap build: %s", err_text(errbits));
    }
    empty_unless_built.armed = false;
    return BK_OK;
}

#if BK_DEBUG_API
/* test hook: the forward build's quad pass on a corner table of the caller's (blinky_hip_debug.h) */
extern "C" int bk_debug_set_forward_corners(bk_ctx *ctx, const int32_t *xy, const uint8_t *ok, size_t ncorners)
{
    if (!ctx) return BK_E_INVALID;
    ctx->clear_debug_corners();
    if (!xy || !ok || !ncorners) return BK_OK;
    ctx->dbg_corner_xy.assign(xy, xy + 2 * ncorners);
    ctx->dbg_corner_ok.assign(ok, ok + ncorners);
    ctx->dbg_corners_set = true;
    return BK_OK;
}
#endif

#if BK_DEBUG_API
extern "C" int bk_debug_forward_tiles(bk_ctx *ctx, int *taken, int *total)
{
    if (!ctx || !taken || !total) return BK_E_INVALID;
    const size_t nt = ((size_t)ctx->ps + 15) / 16, n = (size_t)ctx->numplates * nt * nt;
    *total = (int)n;
    *taken = -1;
    if (!ctx->fwd_tiles_used || !ctx->fwd_tables || ctx->fwd_tables_ps != ctx->ps) return BK_OK;
    std::vector<unsigned char> flags(n);
    const size_t at = 21 * 21 * sizeof(double) + 2 * ((size_t)ctx->ps + 1) * sizeof(float);       // (behind the quotient and uv tables: bk_build)
    BK_HIP(ctx, hipSetDevice(ctx->device));
    BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    BK_HIP(ctx, hipMemcpy(flags.data(), (const char *)ctx->fwd_tables + at, n, hipMemcpyDeviceToHost));
    int k = 0;
    for (unsigned char f : flags) k += f ? 1 : 0;
    *taken = k;
    return BK_OK;
}
#endif

// ---- the seam table (bk_read_seam_table, bk_apply_rgba_fb_bilinear_seams_device) ---------------------------------------------
/* One entry: the texel that stands in for the VIRTUAL texel (x, y) one step outside plate p (x or y is -1 or ps), in the reference
 * layout, or NULL.  The ray through the virtual texel's centre (plate_uv_to_ray, fisheye.c:1198), the plate it selects
 * (ray_to_plate_index, :2023-2050 - the globe's globe_plate where there is one), then set_lensmap_from_ray's position on that plate
 * exactly as bk_inverse_entry / h_inverse_entry take it from the float ray on (:2055-2062, :2065, :1988, :1971).  No grid, no tint. */
static uint32_t seam_entry(bk_ctx *ctx, HostEval &E, const BkBuildParams &bp, int p, int x, int y)
{
    const double u = ((double)x + 0.5) / bp.ps, v = ((double)y + 0.5) / bp.ps;
    float ray[3];
    bk::h_plate_uv_to_ray(ctx->plates[p], u, v, ray);
    const int q = h_ray_to_plate_index(E, bp, ray);
    if (q < 0 || q == p) return BK_NULL_OFFSET;
    const BkPlateDev &t = bp.plates[q];
    const double px_ = (double)h_dot3(t.right, ray), py_ = (double)h_dot3(t.up, ray), pz_ = (double)h_dot3(t.forward, ray);
    const double tu = px_ / pz_ * t.dist64 + 0.5, tv = -py_ / pz_ * t.dist64 + 0.5;
    if (!(tu >= 0 && tu <= 1 && tv >= 0 && tv <= 1)) return BK_NULL_OFFSET;
    const int tx = h_trunc_to_int(tu * bp.ps), ty = h_trunc_to_int(tv * bp.ps);
    if (!(tx >= 0 && tx < bp.ps && ty >= 0 && ty < bp.ps)) return BK_NULL_OFFSET;
    return (uint32_t)q * (uint32_t)(bp.ps * bp.ps) + (uint32_t)ty * (uint32_t)bp.ps + (uint32_t)tx;
}

/* uint32 [6][4][ps + 2]: edge 0 = row y = -1, 1 = row y = ps, 2 = column x = -1, 3 = column x = ps; index = the coordinate along the
 * edge + 1 (0 and ps + 1: the corners, in both edges that meet there).  Plates from numplates on: NULL.  Without a globe_plate callback
 * every step is an IEEE operation; with one the interpreter answers on the host's libm, as it does for flagged pixels (copies of its
 * state on the pool's workers: the context's own is left as it is). */
int bk::seam_table_compute(bk_ctx *ctx, std::vector<uint32_t> &out)
{
    LensProgram *P = bk::prog_of(ctx);
    BkBuildParams bp;
    fill_params(ctx, &bp);
    const int ps = ctx->ps, n1 = ps + 2;
    out.assign((size_t)BK_MAX_PLATES * 4 * n1, BK_NULL_OFFSET);
    const size_t n = (size_t)ctx->numplates * 4 * n1;
    auto one = [&](HostEval &E, size_t k) {
        const int p = (int)(k / (size_t)(4 * n1)), edge = (int)(k / (size_t)n1) & 3, along = (int)(k % (size_t)n1) - 1;
        const int x = edge == 2 ? -1 : edge == 3 ? ps : along, y = edge == 0 ? -1 : edge == 1 ? ps : along;
        out[k] = seam_entry(ctx, E, bp, p, x, y);
    };
    if (!P->globe_plate.is_function()) {
        HostEval E{nullptr, Value(), Value(), Value()};
        for (size_t k = 0; k < n; ++k) one(E, k);
        return BK_OK;
    }
    try {
        for_each_flagged(P, n, one);
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "seam table: %s", e.what());
    }
    return BK_OK;
}

#if BK_DEBUG_API
/* test hook: the kernel-argument block bk_build would launch with (calc_zoom done, device pointers as they are -
 * null on a BK_DEVICE_NONE context).  tests/hostemu compiles the generated translation unit for the host and runs it
 * on this block to inspect the device code's results and flags without a GPU. */
extern "C" int bk_debug_build_params(bk_ctx *ctx, void *out, size_t cap, size_t *needed)
{
    if (!ctx) return BK_E_INVALID;
    if (needed) *needed = sizeof(BkBuildParams);
    if (!out) return BK_OK;
    if (cap < sizeof(BkBuildParams)) return ctx->fail(BK_E_INVALID, "bk_debug_build_params: buffer too small");
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid) return ctx->fail(BK_E_STATE, "not a valid lens");
    if (!ctx->globe_valid) return ctx->fail(BK_E_STATE, "not a valid globe");
    if (int r = bk_calc_zoom(ctx, nullptr)) return r;
    BkBuildParams bp;
    fill_params(ctx, &bp);
    memcpy(out, &bp, sizeof bp);
    return BK_OK;
}
#endif

#if BK_DEBUG_API
/* test hook: the host re-evaluation bk_build applies to flagged pixels, run over ANY pixel indices of the owned rows
 * (works on a BK_DEVICE_NONE context).  offsets come back in the reference layout plate*ps*ps + py*ps + px. */
extern "C" int bk_debug_host_entries(bk_ctx *ctx, const uint32_t *ids, size_t n, uint32_t *offsets, uint8_t *tints)
{
    if (!ctx || !ids || !offsets || !tints) return BK_E_INVALID;
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid || !P->lens_inverse.is_function()) return ctx->fail(BK_E_STATE, "no lens_inverse");
    if (!ctx->globe_valid) return ctx->fail(BK_E_STATE, "not a valid globe");
    if (int r = bk_calc_zoom(ctx, nullptr)) return r;
    BkBuildParams bp;
    fill_params(ctx, &bp);
    const size_t px = (size_t)ctx->W * ctx->rows();
    for (size_t i = 0; i < n; ++i) if (ids[i] >= px) return ctx->fail(BK_E_INVALID, "bk_debug_host_entries: index out of range");
    std::vector<int> shown(n), err(n, 0);
    std::vector<uint16_t> sub(n);                         // (not handed out)
    try {
        std::string src;                                  // (none: the interpreter answers)
        if (bk::g_debug.host_module != 2 && generate_source(ctx, P, &src) != BK_OK) src.clear();
        if (bk::g_debug.host_module == 1 && (src.empty() || !fixup_module(P, src)))
            return ctx->fail(BK_E_STATE, "bk_debug_host_entries: no host module (no C++ compiler, or host math is not the platform libm)");
        rederive(ctx, P, src, ids, 1, n, false,
                 [&](const HostModule &hm, const uint32_t *id, int stride, unsigned long cnt, size_t i) { hm.inverse(&bp, id, stride, cnt, &offsets[i], &tints[i], &sub[i], &shown[i], &err[i]); },
                 [&](HostEval &E, uint32_t id, size_t i) { h_inverse_entry(E, bp, id, &offsets[i], &tints[i], &sub[i], &shown[i], &err[i]); });
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "%s", e.what());
    }
    for (size_t i = 0; i < n; ++i) {
        if (offsets[i] == BK_NULL_OFFSET) continue;
        unsigned plate, x, y;
        bk_texel_coords((unsigned)ctx->gp, (unsigned)ctx->ph, offsets[i], &plate, &x, &y);
        offsets[i] = plate * (unsigned)(ctx->ps * ctx->ps) + y * (unsigned)ctx->ps + x;
    }
    return BK_OK;
}
#endif

#if BK_DEBUG_API
/* the same for the forward build's texel corners (ids: corner number plate * (ps+1)^2 + j * (ps+1) + i): screen x, y and
 * whether lens_forward gave a position */
extern "C" int bk_debug_host_corners(bk_ctx *ctx, const uint32_t *ids, size_t n, int32_t *sx, int32_t *sy, uint8_t *ok)
{
    if (!ctx || !ids || !sx || !sy || !ok) return BK_E_INVALID;
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid || !P->lens_forward.is_function()) return ctx->fail(BK_E_STATE, "no lens_forward");
    if (!ctx->globe_valid) return ctx->fail(BK_E_STATE, "not a valid globe");
    if (int r = bk_calc_zoom(ctx, nullptr)) return r;
    BkBuildParams bp;
    fill_params(ctx, &bp);
    const size_t n1 = (size_t)ctx->ps + 1, total = (size_t)ctx->numplates * n1 * n1;
    for (size_t i = 0; i < n; ++i) if (ids[i] >= total) return ctx->fail(BK_E_INVALID, "bk_debug_host_corners: index out of range");
    std::vector<int> err(n, 0), x(n), y(n);
    try {
        std::string src;                                  // (none: the interpreter answers)
        if (bk::g_debug.host_module != 2 && generate_source(ctx, P, &src) != BK_OK) src.clear();
        if (bk::g_debug.host_module == 1 && (src.empty() || !fixup_module(P, src)))
            return ctx->fail(BK_E_STATE, "bk_debug_host_corners: no host module (no C++ compiler, or host math is not the platform libm)");
        rederive(ctx, P, src, ids, 1, n, false,
                 [&](const HostModule &hm, const uint32_t *id, int stride, unsigned long cnt, size_t i) { hm.corners(&bp, id, stride, cnt, &x[i], &y[i], &ok[i], &err[i]); },
                 [&](HostEval &E, uint32_t id, size_t i) { h_corner_entry(ctx, E, bp, id, &x[i], &y[i], &ok[i], &err[i]); });
    } catch (const LuaError &e) {
        return ctx->fail(BK_E_SCRIPT, "%s", e.what());
    }
    for (size_t i = 0; i < n; ++i) { sx[i] = x[i]; sy[i] = y[i]; }
    return BK_OK;
}
#endif

#if BK_DEBUG_API
extern "C" int bk_debug_build_breakdown(const bk_ctx *ctx, double out[6])
{
    if (!ctx || !out) return BK_E_INVALID;
    out[0] = ctx->last_build_ms;
    out[1] = ctx->last_host_eval_ms;
    out[2] = (double)ctx->last_flagged;
    out[3] = (double)bk::HostPool::get().size();
    out[4] = ctx->last_kernel_wall_ms;
    out[5] = (double)ctx->last_kernel_retries + (ctx->last_fixup_compiled ? 1000.0 : 0.0);
    return BK_OK;
}
#endif

/* Is the compiled host module of the current lens + globe there (see bk_set_host_compile)?  wait != 0: compile it now if need
 * be and wait for it.  1 = ready, 0 = not (still compiling, no compiler, switched off, host math not the platform libm). */
extern "C" int bk_host_module_ready(bk_ctx *ctx, int wait)
{
    if (!ctx) return 0;
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid || !ctx->globe_valid || P->info.map_type == BK_MAP_NONE) return 0;
    if (P->interp.math != &math_platform()) return 0;
    std::string src;
    if (generate_source(ctx, P, &src) != BK_OK) return 0;
    return host_module_for(src, wait != 0) ? 1 : 0;
}

/* Multi-GPU companion of bk_build's handling of a malformed callback result: `bad_key` = the group's first failing pixel
 * (max over the stripes of bk_last_build_bad_key); this stripe gives up what the reference's scan had not reached by then. */
extern "C" unsigned int bk_last_build_bad_key(const bk_ctx *ctx) { return ctx ? ctx->last_bad_key : 0u; }
extern "C" int bk_truncate_build(bk_ctx *ctx, unsigned int bad_key, int display_out[BK_MAX_PLATES])
{
    if (!ctx) return BK_E_INVALID;
    if (!ctx->lensmap_valid || !ctx->d_offsets) return ctx->fail(BK_E_STATE, "bk_truncate_build: no lensmap");
    BK_HIP(ctx, hipSetDevice(ctx->device));
    bk::resident_quiesce(ctx);
    int disp[BK_MAX_PLATES];
    if (bad_key == 0) return BK_OK;
    if (int r = bk::launch_truncate_scan(ctx, bad_key, disp)) return r;
    ctx->last_bad_key = bad_key;
    bk::lensmap_edited(ctx);                          // (the pass took the plane along where it is valid: its flag stays)
    for (int i = 0; i < BK_MAX_PLATES; ++i) { ctx->display[i] = i < ctx->numplates ? disp[i] : 0; if (display_out) display_out[i] = ctx->display[i]; }
    return BK_OK;
}

extern "C" int bk_last_build_fixups(const bk_ctx *ctx, int *flagged, int *changed)
{
    if (!ctx) return BK_E_INVALID;
    if (flagged) *flagged = ctx->last_flagged;
    if (changed) *changed = ctx->last_changed;
    return BK_OK;
}

// debug / test hook: run a callback on the DEVICE over n argument tuples (nargs doubles each);
// out receives 8 doubles per tuple, nout the result count (-1 single nil, <= -100 runtime error)
/* f_saveglobe's plate image (fisheye.c:1438-1456), computed on the device; the caller encodes the PCX */
extern "C" int bk_save_plate(bk_ctx *ctx, int frame, int plate, int with_margins, uint8_t *dst_host, int dst_pitch)
{
    if (!ctx || !dst_host) return BK_E_INVALID;
    if (ctx->device < 0) return ctx->fail(BK_E_STATE, "bk_save_plate: this context has no device");
    if (!ctx->d_globe) return ctx->fail(BK_E_STATE, "bk_save_plate: call bk_resize first");
    if (!ctx->globe_valid || !ctx->prog) return ctx->fail(BK_E_STATE, "not a valid globe");
    if (plate < 0 || plate >= ctx->numplates || frame < 0 || frame >= ctx->nframes || dst_pitch < ctx->ps)
        return ctx->fail(BK_E_INVALID, "bk_save_plate: bad frame/plate/pitch");
    BK_HIP(ctx, hipSetDevice(ctx->device));
    bk::resident_quiesce(ctx);
    LensProgram *P = ctx->prog;
    std::string src;
    if (int r = generate_source(ctx, P, &src)) return r;
    if (int r = compile_module(ctx, P, src)) return r;
    hipFunction_t fn = nullptr;
    BK_HIP(ctx, hipModuleGetFunction(&fn, P->module, "bk_save_plate"));
    if (int r = alloc_flag_buffers(ctx)) return r;
    const uint8_t *globe = ctx->d_globe + (size_t)frame * ctx->globe_stride();
    uint8_t *out = nullptr;
    BK_HIP(ctx, hipMalloc((void **)&out, (size_t)ctx->ps * ctx->ps));
    const DeviceMem out_mem(out);
    BkBuildParams bp;
    fill_params(ctx, &bp);
    void *args[] = {&bp, &plate, &with_margins, &globe, &out};
    int counters[kNumCounters];
    std::vector<uint32_t> flagged;
    if (int r = flagged_pass(ctx, "bk_save_plate", bp, true, [&] {
            return hipModuleLaunchKernel(fn, (unsigned)((ctx->ps + 255) / 256), (unsigned)ctx->ps, 1, 256, 1, 1, 0, ctx->stream, args, nullptr);
        }, counters, &flagged)) return r;
    hipError_t e = hipMemcpy2DAsync(dst_host, (size_t)dst_pitch, out, (size_t)ctx->ps, (size_t)ctx->ps, (size_t)ctx->ps, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ctx->fail(BK_E_HIP, "bk_save_plate failed: %s", hipGetErrorString(e));
    // texels whose plate ownership a globe_plate script decides on libm's last bits: the host interpreter has the say
    if (!flagged.empty()) {
        const size_t nfl = flagged.size() / 4;
        std::vector<uint8_t> own(nfl);
        try {
            for_each_flagged(P, nfl, [&](HostEval &E, size_t k) {
                const uint32_t id = flagged[4 * k], i = id / (uint32_t)ctx->ps, j = id - i * (uint32_t)ctx->ps;
                float ray[3];
                bk::h_plate_uv_to_ray(ctx->plates[plate], (double)j / ctx->ps, (double)i / ctx->ps, ray);
                own[k] = plate == h_ray_to_plate_index(E, bp, ray);
            });
        } catch (const LuaError &err) {
            return ctx->fail(BK_E_SCRIPT, "%s", err.what());
        }
        for (size_t k = 0; k < nfl; ++k) {
            const uint32_t id = flagged[4 * k], i = id / (uint32_t)ctx->ps, j = id - i * (uint32_t)ctx->ps;
            dst_host[(size_t)i * dst_pitch + j] = own[k] ? (uint8_t)flagged[4 * k + 1] : 0xFE;
        }
    }
    return BK_OK;
}

#if BK_DEBUG_API
static int eval_device(bk_ctx *ctx, int which, const double *args, int nargs, int n, double *out, int *nout, double *bound, int *flag)
{
    if (!ctx || !args || !out || !nout || nargs < 1 || nargs > 4 || n < 1) return BK_E_INVALID;
    if (ctx->device < 0) return ctx->fail(BK_E_STATE, "this context has no device");
    LensProgram *P = ctx->prog;
    if (!P || !P->lens_valid) return ctx->fail(BK_E_STATE, "no valid lens");
    BK_HIP(ctx, hipSetDevice(ctx->device));
    bk::resident_quiesce(ctx);
    std::string src;
    if (int r = generate_source(ctx, P, &src)) return r;
    if (int r = compile_module(ctx, P, src)) return r;
    hipFunction_t fn = nullptr;
    BK_HIP(ctx, hipModuleGetFunction(&fn, P->module, "bk_eval_callback"));
    BkBuildParams bp;
    fill_params(ctx, &bp);
    // one allocation: args [n * nargs], out [8 n], bound [8 n] (doubles), then nout [n], flag [n] (ints)
    // (the ints come last, so every region is aligned for its type; bound and flag are laid out whether or not the caller reads them)
    const size_t nd = (size_t)n * (size_t)(nargs + 16);
    double *d_args = nullptr;
    BK_HIP(ctx, hipMalloc((void **)&d_args, sizeof(double) * nd + sizeof(int) * 2 * (size_t)n));
    const DeviceMem mem(d_args);
    double *d_out = d_args + (size_t)n * nargs, *d_bound = d_out + (size_t)n * 8;
    int *d_nout = (int *)(d_bound + (size_t)n * 8), *d_flag = d_nout + n;
    double *k_bound = bound ? d_bound : nullptr;
    int *k_flag = flag ? d_flag : nullptr;
    BK_HIP(ctx, hipMemcpyAsync(d_args, args, sizeof(double) * nargs * n, hipMemcpyHostToDevice, ctx->stream));
    void *kargs[] = {&bp, &which, &d_args, &nargs, &n, &d_out, &d_nout, &k_bound, &k_flag};
    hipError_t e = hipModuleLaunchKernel(fn, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, ctx->stream, kargs, nullptr);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, sizeof(double) * 8 * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(nout, d_nout, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && bound) e = hipMemcpyAsync(bound, d_bound, sizeof(double) * 8 * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && flag) e = hipMemcpyAsync(flag, d_flag, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);         // (always, before the buffer goes)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return ctx->fail(BK_E_HIP, "bk_debug_eval_device: %s", hipGetErrorString(e));
    return BK_OK;
}
extern "C" int bk_debug_eval_device(bk_ctx *ctx, int which, const double *args, int nargs, int n, double *out, int *nout)
{
    return eval_device(ctx, which, args, nargs, n, out, nout, nullptr, nullptr);
}
extern "C" int bk_debug_eval_device_bounds(bk_ctx *ctx, int which, const double *args, int nargs, int n, double *out, double *bound, int *flag,
                                           int *nout)
{
    if (!bound || !flag) return BK_E_INVALID;
    return eval_device(ctx, which, args, nargs, n, out, nout, bound, flag);
}
#endif
