// bk_internal.h -- private state of libblinkyhip.so (see include/blinky_hip.h for the ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "../../include/blinky_hip.h"
#ifndef BK_DEBUG_API
#define BK_DEBUG_API 0
#endif
#if BK_DEBUG_API
#include "../../include/blinky_hip_debug.h"
#endif
#include "bk_build_params.h"      // the device globe layout (bk_texel_offset)

namespace bk {

// process-wide developer / test switches (bk_debug_set_option, debug API builds only; always 0 otherwise)
struct DebugOptions { int no_memcache = 0, libm_rel_log2 = 0, print_model = 0, host_module = 0, no_direct_submit = 0, forward_careful = 0; };
extern DebugOptions g_debug;

// roctx ranges around the library's phases (bk_build, block-map compile, apply launches, plate uploads, the resident session):
// `rocprofv3 --marker-trace --kernel-trace` then groups the kernels by phase instead of by name.
// libroctx64 is resolved with dlopen on first use; without it (or without a profiler attached) a range costs two indirect calls.
struct Range {
    explicit Range(const char *name);
    ~Range();
    Range(const Range &) = delete;
    Range &operator=(const Range &) = delete;
};

// A run of mapped pixels in one output row (host-side, for merging a warped
// frame into the caller's vid.buffer without touching unmapped pixels).
struct Span { int row, x0, x1; };

struct Rubix { int numcells = 10; double cell = 4, pad = 1; };   // defaults: fisheye.c:672

// The device copy of a palette or of a truecolour launch's byte LUTs, kept while the bytes AND the stream are the same (an upload is
// ordered with the launches of the stream it was issued on only).  A context has three, each its own buffer and cache, so that none
// disturbs another's: the 8-bit palette (bk_apply*), the staged truecolour applies' LUTs, the frame-buffer applies' LUTs.
struct LutCopy {
    uint8_t *d = nullptr;                         // allocated by the first upload
    uint8_t host[4 * BK_MAX_PLATES * 256] = {};   // what d holds, uploaded on `stream` (the palette: the first quarter)
    hipStream_t stream = nullptr;
    bool cached = false;
    int upload(bk_ctx *ctx, const void *src, size_t bytes);      // bk_api.cpp; bytes <= sizeof host, the same for every call
    void free() { (void)hipFree(d); d = nullptr; cached = false; }
};

struct LensProgram;   // bk_lens_priv.h: parsed scripts + hiprtc modules
struct CoopMap;       // bk_apply_coop.hip: per-block staging plans of the workgroup-cooperative apply kernel
struct Resident;      // bk_apply_resident.inc: the resident single-frame apply (its kernel, command ring and stream)

}  // namespace bk

struct bk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // geometry (fisheye.c:704-708)
    int W = 0, H = 0, ps = 0;
    int gp = 0, ph = 0;              // padded plate width round_up(ps, 64) / height round_up(ps, 8) of the device globe
    int row0 = 0, row1 = 0;          // owned output rows
    int nframes = 1;

    // globe (fisheye.c:334-377)
    bk_plate plates[BK_MAX_PLATES] = {};
    int numplates = 0;
    bool globe_valid = false;
    int display[BK_MAX_PLATES] = {};

    // zoom / rubix (fisheye.c:453-474)
    int zoom_type = BK_ZOOM_NONE, zoom_fov = 0;
    double scale = -1;
    bk::Rubix rubix;

    // device memory
    uint8_t *d_globe = nullptr;      // [nframes][6][ph/8][gp/16] tiles of 16x8 texels (bk_texel_offset, bk_build_params.h)
    uint8_t *d_plate_stage = nullptr;  // [ps][gp] row-major staging of one plate for bk_upload_plate / bk_download_plate
    uint8_t *d_rgba_stage = nullptr;   // [ps][4*ps] one truecolour plate on its way from the host (bk_upload_plate_rgba); allocated on first use
    size_t rgba_stage_bytes = 0;
    // the footprint of the lensmap (bk_plate_footprint, bk_upload_plate_rgba_footprint*): bit t of d_fp_bits = "some entry of the owned rows
    // reads 128-byte tile t of a globe slot" (t = device offset >> 7, plates back to back); computed on the first query after the lensmap
    // changed (launch_footprint), never by a build.  h_fp (pinned) = the same bits, then 5 ints per plate: tiles read, x0, y0, x1, y1 of
    // their bounding box in tiles (half-open; all 0 when nothing is read)
    uint32_t *d_fp_bits = nullptr;
    uint32_t *h_fp = nullptr;
    size_t fp_words = 0;               // uint32 words of the bitmap the two buffers were allocated for
    bool footprint_valid = false;
    // bk_upload_plate_async: pinned host buffers the caller's rows are copied into, their device-side staging twins and
    // the event that says "this slot's DMA + retile are done" - three slots, so that the DMA of plate k overlaps the
    // engine's render of plate k+1
    static constexpr int kPlateSlots = 3;
    uint8_t *h_plate[kPlateSlots] = {};
    uint8_t *d_plate_slot[kPlateSlots] = {};
    hipEvent_t plate_ev[kPlateSlots] = {};
    size_t plate_slot_bytes = 0;
    int plate_next = 0;
    uint32_t *d_offsets = nullptr;   // [row1-row0][W]  offsets into the PADDED globe layout
    uint32_t *d_convert = nullptr;   // [row1-row0][W]  scratch for layout conversion at the ABI boundary
    uint8_t *d_tints = nullptr;      // [row1-row0][W]
    // bk_set_subtexel: [row1-row0][W] where inside its texel each mapped pixel's ray landed (qx | qy << 8, 0x8080 = centre; BkBuildParams::subtexel).
    // Allocated by the first bk_build / bk_set_lensmap / bk_set_lensmap_subtexel with the switch on, freed with the maps or by switching off;
    // subtexel_valid: it describes the lensmap in place (lives and dies with lensmap_valid)
    uint16_t *d_subtexel = nullptr;
    bool subtexel_on = false, subtexel_valid = false;
    // the seam table (bk_read_seam_table / bk_set_seam_table / bk_apply_rgba_fb_bilinear_seams_device): uint32 [6][4][ps + 2] in the
    // reference layout, the texels that stand in for the virtual ones a step outside every plate.  Made on the host on first use
    // (bk::seam_table_ready) or set by the caller (seam_user), never by a build; dropped (bk::seam_drop) by whatever can change the
    // plates, the platesize or the globe_plate root.  d_seam = its decoded device form, uint2 [6][4][ps + 2] = {plate * gp * ph or
    // 0xFFFFFFFF, py << 16 | px}, uploaded once per table (d_seam_current) into a buffer of d_seam_words entries
    std::vector<uint32_t> seam_table;
    bool seam_valid = false, seam_user = false;
    uint2 *d_seam = nullptr;
    size_t d_seam_words = 0;
    bool d_seam_current = false;
    // the trilinear frame-buffer apply (bk_apply_rgba_mip.inc).  d_lod: the level-of-detail plane, uint16 [row1-row0][W] = level << 8 | fraction,
    // beside the maps (map_px entries; freed with them), allocated by the first bk_read_lod / bk_set_lensmap_lod / trilinear apply;
    // lod_state: 0 = to be derived, 1 = derived, 2 = set by the caller - back to 0 (bk::lod_invalidate) whenever the lensmap, the
    // sub-texel plane, the owned rows or lod_bias change; never touched by a build.
    // d_mip: the table (BK_MIP_TABLE_BYTES: mip_table as uint4 [16]) and levels 1 .. mip_levels - 1 of the six plates, mip_plate_stride bytes
    // each, for platesize mip_ps; allocated by the first trilinear apply with mips = 1, freed by a bk_resize that changes ps and by
    // bk_destroy; mip_made: that pyramid has been filled at least once
    uint16_t *d_lod = nullptr;
    int lod_state = 0, lod_bias = 0;
    uint8_t *d_mip = nullptr;
    int mip_ps = 0, mip_levels = 0;
    bool mip_made = false;
    size_t mip_plate_stride = 0;
    uint32_t mip_table[BK_MIP_MAX_LEVELS][4] = {};      // {byte offset inside a plate's part, row pitch, s_k - 1, s_k}
    uint8_t *d_frame = nullptr;      // [row1-row0][W] staging for bk_apply (host dst)
    bk::LutCopy pal;                 // [6][256] the 8-bit palette (upload_pal); its buffer is there from bk_create on
    bk::LutCopy lut_rgba;            // [4][6][256] the byte LUTs of bk_apply_rgba_tinted_device / _ss2_device (pal stays the 8-bit palette)
    bk::LutCopy lut_fb;              // [4][6][256] the byte LUTs of the frame-buffer applies
    uint64_t *d_mask = nullptr;      // mapped bits, 1 per pixel of the owned rows
    int *d_display = nullptr;        // [6] display flags + [1] error bits + [1] flagged-entry count + [1] first malformed result (scan key + 1) written by the build kernels
    unsigned int last_bad_key = 0;   // of the last bk_build: 1 + scan key of the first pixel whose callback returned a malformed result (0 = none)
    uint32_t *d_flag_list = nullptr; // entries a build flagged for re-evaluation on the platform libm (bk_device_rt.h)
    size_t flag_cap = 0;
    // scratch of the forward build, kept from one build to the next (four hipMalloc / hipFree of 320 MB at 4K cost more wall time than
    // its kernels): texel-corner screen coordinates, corner flags, the two key planes; released when an inverse map is built
    void *fwd_scratch[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t fwd_scratch_bytes[4] = {0, 0, 0, 0};
    // fill_params' rubix grid bitmap for (platesize, rubix numcells / cell / pad): a division and an fmod per texel column, once - not per build
    unsigned int grid_cache[256] = {0};
    double grid_cache_key[4] = {-1, 0, 0, 0};
    hipStream_t build_aux = nullptr;     // a forward build clears its key planes here, beside the corner pass
    hipEvent_t build_ev[2] = {nullptr, nullptr};
    hipEvent_t build_time_ev[2] = {nullptr, nullptr};   // bk_build's timing pair, kept (creating and destroying them is four runtime calls a build)
    int *h_build_flags = nullptr;        // pinned: the counters of a forward build's two passes, read back without a stop in between
    bool fwd_tiles_used = false;         // the last build's quad pass went by bk_forward_tiles' flags (bk_debug_forward_tiles)
    void *fwd_tables = nullptr;          // BkBuildParams::fwd_quot + fwd_uv for platesize fwd_tables_ps (bk_build.cpp)
    int fwd_tables_ps = -1;
    // bk_debug_set_forward_corners (tests): a host copy of a texel-corner table that the forward build on the device uploads in place
    // of its corner pass
#if BK_DEBUG_API
    std::vector<int32_t> dbg_corner_xy;
    std::vector<uint8_t> dbg_corner_ok;
    bool dbg_corners_set = false;
    void clear_debug_corners() { dbg_corner_xy.clear(); dbg_corner_ok.clear(); dbg_corners_set = false; }
    bool debug_corners_set() const { return dbg_corners_set; }
#else
    void clear_debug_corners() {}
    bool debug_corners_set() const { return false; }
#endif
    int last_flagged = 0, last_changed = 0;   // of the last bk_build: entries re-evaluated on the host / entries that changed
    uint8_t *h_frame = nullptr;      // pinned, [row1-row0][W]
    uint64_t *h_mask = nullptr;      // pinned
    size_t globe_bytes = 0;          // allocated size of d_globe
    size_t map_px = 0;               // allocated pixels for the map buffers

    bool lensmap_valid = false;
    std::vector<bk::Span> spans;     // mapped spans of the owned rows
    bool spans_valid = false;
    bool apply_in_flight = false;    // between bk_apply_begin and bk_apply_end
    bool fully_mapped = false;       // every pixel of the owned rows is mapped: bk_apply copies the frame whole

    int apply_variant = -1;          // -1 auto (= 2); 0 direct gather, 2 workgroup-cooperative LDS blocks
    int num_cus = 256;               // multiProcessorCount of the device
    int apply_flags = 0;             // developer ablations of the coop apply (bk_debug_set_ablation): 2 no globe loads, 4 no stores, 8 no load pipelining
                                     // ... (BkAblation, bk_apply_coop.hip).  A resident session reads the same word its own way (BkResidentFlag):
                                     // 4 no stores, 8 every frame on its own, 16 no frame stride, 2048 not the one-block form, 4096 no table
                                     // forms, 8192 time every workgroup's frames; its kernel is handed 4 | 8 | 8192 of them and nothing else
    int apply_block_cost = -1;       // coop apply: constant term of a block's cost in the band balance (-1 = default; knob 600+n)
    int apply_lds_kb = 0;            // coop apply: force the staging buffer size in KiB (0 = cost model; knob 400+n)
    int apply_fchunk = 0;            // frames a workgroup keeps a block for (0 = default 8; knob 300+n)
    int apply_wgs_per_cu = 16;       // persistent apply grid: workgroups per CU (tunable, bk_debug_set_tile_shape)
    bool blockmap_tuning = true;     // bk_set_blockmap_tuning: block height of the staged apply chosen by timing the candidates
    int tile_shape = 0;              // coop apply: 0 = block height by cost model, 1/2/4 = force 128x8 / 128x16 / 128x32
    bk::CoopMap *coopmap = nullptr;       // owned; freed with bk::coopmap_free
    bk::CoopMap *coopmap_alt = nullptr;   // owned: the block map of the OTHER flavour (plain / tinted), parked while f_rubix is the other way
    bk::Resident *resident = nullptr;     // owned; freed with bk::resident_free (bk_apply_resident_begin .. _end)
    int resident_mode = 0;                // bk_set_resident_apply: bk_apply / bk_apply_begin..end / bk_upload_plate* go through the resident kernel
    int res_part = 0, res_parts = 1, res_reserve = 0;   // bk_set_resident_share: which CUs of every XCD the resident kernel may take
    uint64_t apply_ticket = 0;            // resident mode: the frame bk_apply_begin submitted
    uint8_t res_pal[BK_MAX_PLATES * 256] = {};   // resident mode: the palette the running session was begun with
    bool res_rubix = false;
    bool apply_was_resident = false;      // latched by bk_apply_begin: the frame in flight went to the resident kernel
    bk::LensProgram *prog = nullptr;      // owned; freed with bk::lensprogram_free
    double last_build_ms = 0;
    double last_host_eval_ms = 0;    // of that: wall time of the host re-evaluation of the flagged entries
    double last_kernel_wall_ms = 0;  // inverse build: wall time of the kernel launch(es) + counter / flag-list read-back (sorted)
    int last_kernel_retries = 0;     // kernel re-runs because the flag list had to grow
    bool last_fixup_compiled = false;   // the flagged entries were re-derived by the compiled host module (not the interpreter)
    uint32_t *host_sink_off = nullptr; uint8_t *host_sink_tint = nullptr;   // bk_debug_host_build: a host-built table goes here instead of the device
    uint16_t *host_sink_sub = nullptr;                                      // ... and its sub-texel plane (bk_debug_host_build_subtexel; nullable)
    int last_build_path = 0;         // of the last bk_build: 0 = GPU kernels, 1 = host worker pool, 2 = one sequential host scan (bk_last_build_path)
    std::string last_build_why;
    int sequential_build = 1;        // bk_set_sequential_build: 0 never, 1 (default) when the callbacks carry state from pixel to pixel, 2 always
    bool async_compile = false;      // bk_set_async_compile: bk_build returns BK_PENDING instead of waiting for hiprtc

    int fail(int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)))
    {
        char buf[2048];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    int rows() const { return row1 - row0; }
    size_t plate_bytes() const { return (size_t)gp * ph; }
    size_t globe_stride() const { return (size_t)BK_MAX_PLATES * gp * ph; }
    size_t plate_tiles() const { return (size_t)(gp >> 4) * (ph >> 3); }      // 16x8-texel tiles (128-byte lines) of a plate, padding included
    const int *fp_summary(int plate) const { return reinterpret_cast<const int *>(h_fp + fp_words) + 5 * plate; }   // valid while footprint_valid
};

#define BK_HIP(ctx, expr)                                                               \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return (ctx)->fail(BK_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace bk {

// bk_apply.hip
int launch_apply(bk_ctx *ctx, int frame0, int nframes, uint8_t *dst_first_owned_row, int dst_pitch,
                 size_t frame_stride, int rubix_on);
int launch_mask(bk_ctx *ctx);                 // d_offsets -> d_mask
int launch_fill_lcg(bk_ctx *ctx, uint8_t *plate_dst, uint32_t seed);   // one plate, padded rows
int launch_convert_offsets(bk_ctx *ctx, uint32_t *buf, size_t n, int to_device);   // reference <-> device (tiled) layout
int launch_plate_retile(bk_ctx *ctx, uint8_t *plate_tiled, int to_tiled, uint8_t *rowmajor = nullptr);   // row-major staging (default d_plate_stage) <-> a plate of the globe
// a row-major plate of 32-bit texels (device memory, rows src_pitch bytes apart) -> the same plate of four consecutive globe slots,
// byte c of every texel into slot c's tiles; plane0 = the plate in the first of the four slots
int launch_plate_rgba_retile(bk_ctx *ctx, uint8_t *plane0, const uint8_t *src_dev, size_t src_pitch);
// the lensmap's footprint (bk_ctx::d_fp_bits / h_fp) if it is not the current one: mark, reduce, ONE host synchronisation
int launch_footprint(bk_ctx *ctx);
inline void footprint_invalidate(bk_ctx *ctx) { ctx->footprint_valid = false; }      // wherever the lensmap or the owned rows change
// the sub-texel plane for the current owned rows, allocated if the switch is on and it is not there yet (bk_api.cpp)
int subtexel_alloc(bk_ctx *ctx);
void footprint_free(bk_ctx *ctx);
// launch_plate_rgba_retile for the tiles of `plate` in the footprint only (which must be current and not empty for that plate)
int launch_plate_rgba_retile_footprint(bk_ctx *ctx, int plate, uint8_t *plane0, const uint8_t *src_dev, size_t src_pitch);
int launch_scatter32(bk_ctx *ctx, uint32_t *dst, const uint32_t *h_idx, const uint32_t *h_val, size_t n);   // dst[idx[i]] = val[i]; synchronous
int launch_scatter8(bk_ctx *ctx, uint8_t *dst, const uint32_t *h_idx, const uint8_t *h_val, size_t n);
int launch_scatter16(bk_ctx *ctx, uint16_t *dst, const uint32_t *h_idx, const uint16_t *h_val, size_t n);
// the owned rows of the lensmap as the reference leaves them when its scan stops at the pixel with scan key bad_key - 1 (everything it
// had not reached yet NULL) and the display flags of what is left; synchronous
int launch_truncate_scan(bk_ctx *ctx, unsigned int bad_key, int display_out[BK_MAX_PLATES]);
// bk_apply_coop.hip
void coopmap_invalidate(bk_ctx *ctx);
// ---- what follows the lensmap: the sub-texel plane beside it and what is made from its entries on first use - the spans, the block
// map, the footprint.  Every change of the table goes through one of these three; a new plane or cache joins them here, nowhere else.
// (coopmap_invalidate ends a resident session and takes a context with no block map, or no device, as it is)
// the entries in place changed, the plane (if valid) with them: bk_truncate_build, whose pass writes the plane only while it is
// valid - so the plane's flag is not lensmap_replaced's formula there
inline void lod_invalidate(bk_ctx *ctx) { ctx->lod_state = 0; }      // the level-of-detail plane, a caller-set one too, no longer describes the lensmap
inline void lensmap_edited(bk_ctx *ctx) { ctx->spans_valid = false; coopmap_invalidate(ctx); footprint_invalidate(ctx); lod_invalidate(ctx); }
// there is no table now (free_maps, empty_context, bk_resize, bk_set_rows): every consumer answers BK_E_STATE until there is one
inline void lensmap_dropped(bk_ctx *ctx) { ctx->lensmap_valid = ctx->subtexel_valid = false; lensmap_edited(ctx); }
// the table in place is new (bk_set_lensmap; bk_build, in front of every way out); its plane, where there is one, was written with it
inline void lensmap_replaced(bk_ctx *ctx) { ctx->lensmap_valid = true; ctx->subtexel_valid = ctx->d_subtexel != nullptr; lensmap_edited(ctx); }
int launch_apply_coop(bk_ctx *ctx, int frame0, int nframes, uint8_t *dst_first_owned_row, int dst_pitch,
                      size_t frame_stride, int rubix_on);
// bk_apply_rgba.inc (part of bk_apply_coop.hip): truecolour frames from truecolour globes (four ring slots each);
// d_lut = nullptr: the plain launch, else the tinted one through the device copy of uint8 [4][BK_MAX_PLATES][256];
// ss2: 2x2 supersampling into half-size frames (bk_apply_rgba_ss2_device) - dst is then row row0 / 2 of the half-size frame
int launch_apply_rgba(bk_ctx *ctx, int globe0, int nframes, uint8_t *dst_first_owned_row, int dst_pitch, size_t frame_stride,
                      const uint8_t *d_lut = nullptr, bool ss2 = false);
// bk_apply_rgba_fb.inc (part of bk_apply_coop.hip): one truecolour frame straight out of six row-major 32-bit plates in device memory
// (a NULL plate: one that no lensmap entry of the owned rows names); dst = the first owned row at the origin.  FB_SS2: of the half-size
// frame; FB_BILINEAR: every pixel blended from the four texels around its sub-texel position (ctx->d_subtexel, which must be there);
// FB_BILINEAR_SEAMS: with the four positions resolved one by one, those outside the plate through ctx->d_seam (which must be current)
enum FbMode { FB_NEAREST, FB_SS2, FB_BILINEAR, FB_BILINEAR_SEAMS };
int launch_apply_rgba_fb(bk_ctx *ctx, const void *const plates[BK_MAX_PLATES], const int pitches[BK_MAX_PLATES], uint8_t *dst, int dst_pitch,
                         const uint8_t *d_lut, FbMode mode);
// bk_apply_rgba_mip.inc (part of bk_apply_coop.hip): the mip pyramid of six frame-buffer plates, the level-of-detail plane and the trilinear apply
#define BK_MIP_TABLE_BYTES 256      // uint4 [BK_MIP_MAX_LEVELS] in front of the pyramid
// levels of a platesize: s_0 = ps, s_{k+1} = (s_k + 1) / 2 down to 1 (0 for ps < 1; at most BK_MIP_MAX_LEVELS for every ps bk_resize accepts)
inline int mip_level_count(int ps) { int n = 0; for (int s = ps; s >= 1; s = (s + 1) / 2) { ++n; if (s == 1) break; } return n; }
int launch_mip_pyramid(bk_ctx *ctx, const void *const plates[BK_MAX_PLATES], const int pitches[BK_MAX_PLATES]);
int launch_lod(bk_ctx *ctx);
int launch_apply_rgba_fb_trilinear(bk_ctx *ctx, const void *const plates[BK_MAX_PLATES], const int pitches[BK_MAX_PLATES], uint8_t *dst, int dst_pitch,
                                   const uint8_t *d_lut);
int coopmap_stats(bk_ctx *ctx, int out[6]);   // blocks, direct-gather blocks, empty blocks, LDS bytes per buffer
int coopmap_traffic_model(bk_ctx *ctx, uint64_t out[8]);
int coopmap_xcd_probe(bk_ctx *ctx, int *out, int nwg);
int coopmap_band_balance(bk_ctx *ctx, uint32_t out[18]);
int coopmap_row_costs(bk_ctx *ctx, uint32_t *rows_out);      // device uint32 [rows()]: block costs spread over their rows, x16
}
int bk_row_costs_device(bk_ctx *ctx, uint32_t *cost_dev);     // bk_probe.hip: what every owned row costs the apply, into a device uint32 [H]
namespace bk {
void coopmap_free(CoopMap *);
// bk_apply_resident.inc (part of bk_apply_coop.hip): the resident single-frame apply
int resident_begin(bk_ctx *ctx, int rubix_on, double idle_ms);
int resident_submit(bk_ctx *ctx, int frame, uint8_t *dst_first_owned_row, int dst_pitch, uint64_t *ticket);
int resident_wait(bk_ctx *ctx, uint64_t ticket, double *gpu_us);
int resident_stop(bk_ctx *ctx);          // the kernel leaves (outstanding frames are finished first); begin again to resume
void resident_free(bk_ctx *ctx);
int resident_info(bk_ctx *ctx, int out[12]);
// every other device entry point of a context calls this first: a resident kernel fills the chip, whatever else the context
// launches would wait for it to leave
inline void resident_quiesce(bk_ctx *ctx) { if (ctx->resident) (void)resident_stop(ctx); }
bool resident_leaves_room(bk_ctx *ctx);
void hw_queue_note();      // one line on stderr, once, when GPU_MAX_HW_QUEUES could not be raised for the resident apply (bk_api.cpp)
/* job(i) for i in [0, parts) on the library's pool of host threads (bk_hostpool.cpp: the pool that re-derives flagged pixels), the caller
 * waiting; parts <= 1 or a pool of one thread: on the calling thread */
void host_parallel(size_t parts, const std::function<void(size_t)> &job);
bool resident_running(bk_ctx *ctx);      // a session's kernel is on the device right now

// bk_lens.cpp
void lensprogram_free(LensProgram *);
// BK_OK when the current lens + globe's kernels are loaded (or were found in a cache just now), BK_PENDING while hiprtc is
// still compiling them on another thread (asynchronous compilation only; nothing of the context's lensmap is touched)
int build_module_ready(bk_ctx *ctx);
// bk_api.cpp
void empty_context(bk_ctx *ctx);
// the seam table: forget it (a caller-set one too); make sure ctx->seam_table is there (who = the caller's name for messages)
inline void seam_drop(bk_ctx *ctx) { ctx->seam_valid = ctx->seam_user = ctx->d_seam_current = false; }
int seam_table_ready(bk_ctx *ctx, const char *who);
// bk_build.cpp: the table for the globe and platesize in place, uint32 [6][4][ps + 2], on the host
int seam_table_compute(bk_ctx *ctx, std::vector<uint32_t> &out);

}  // namespace bk
