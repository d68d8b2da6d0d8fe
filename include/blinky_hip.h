/*
 * blinky_hip.h -- C ABI of libblinkyhip.so: the MI355X (gfx950) implementation of
 * Blinky's globe->screen warp (lensmap build + per-frame lensmap apply).
 *
 * The reference has no FFI for this path: engine/NQ/fisheye.c is one C
 * translation unit of static functions (engine/include/fisheye.h:4-9 is its
 * whole public face).  This header is the seam a maintainer binds instead of
 * those statics; every entry point names the reference code it replaces
 * (paths relative to /root/reference/engine).  Plain C types only; the host
 * side (blinky_amd/host/fisheye_hip.c) stays C, exactly like the reference.
 *
 * Conventions
 *   - every int-returning function returns BK_OK (0) or a negative BK_E_* code;
 *     bk_last_error() gives the message (the reference's Con_Printf text where
 *     one exists).  Nothing ever exit()s (the reference does on OOM, fisheye.c:723-726).
 *   - a lensmap entry is offset = ptr - globe.pixels = plate*ps*ps + py*ps + px
 *     (GLOBEPIXEL, fisheye.c:349) as uint32, BK_NULL_OFFSET for a NULL pointer;
 *     tints are the bytes of lens.pixel_tints (255 = none, fisheye.c:432-449).
 *   - all device work is enqueued on the context's HIP stream (bk_set_stream);
 *     host-pointer entry points are synchronous with respect to their buffers.
 *   - there is no CPU fallback: without a usable GPU bk_create fails.
 *   - texels and pixels are 8-bit palettised, as the reference's (TyrQuake's software rasteriser).  TRUECOLOUR - 32-bit plates
 *     warped into 32-bit frames, for hosts whose plates are frame buffers of a present-day renderer - is bk_upload_plate_rgba /
 *     bk_upload_plate_rgba_device / bk_plate_footprint / bk_upload_plate_rgba_footprint / bk_upload_plate_rgba_footprint_device /
 *     bk_apply_rgba_device / bk_apply_rgba_tinted_device / bk_apply_rgba_ss2_device / bk_apply_rgba_fb_device (one frame straight out
 *     of the frame buffers, no globe at all): a 32-bit globe is four byte planes in four consecutive slots of the same
 *     globe ring, so lens build, lensmap and everything else in this header are shared with the 8-bit path as they are.
 */
#ifndef BLINKY_HIP_H
#define BLINKY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BK_MAX_PLATES   6             /* MAX_PLATES, fisheye.c:352 */
#define BK_NULL_OFFSET  0xFFFFFFFFu
#define BK_DEVICE_NONE  (-2)          /* bk_create: host-only context (scripts, zoom, code generation) */

enum {
    BK_PENDING = 1,        /* bk_build with bk_set_async_compile: the lens is still compiling, call again later */
    BK_OK = 0,
    BK_E_INVALID = -1,     /* bad argument / call order */
    BK_E_HIP = -2,         /* HIP runtime or hiprtc failure (message has the detail) */
    BK_E_SCRIPT = -3,      /* lens / globe script failed to load, run or compile */
    BK_E_ZOOM = -4,        /* calc_zoom() failure (fisheye.c:1293-1386) */
    BK_E_NOMEM = -5,
    BK_E_STATE = -6        /* no valid lens/globe/lensmap for the requested operation */
};

enum { BK_MAP_NONE = 0, BK_MAP_INVERSE = 1, BK_MAP_FORWARD = 2 };                 /* fisheye.c:391 */
enum { BK_ZOOM_NONE = 0, BK_ZOOM_FOV, BK_ZOOM_VFOV, BK_ZOOM_COVER, BK_ZOOM_CONTAIN }; /* fisheye.c:457 */

typedef struct bk_ctx bk_ctx;

/* One globe plate as LUA_load_globe leaves it (fisheye.c:353-361, 1796-1869). */
typedef struct {
    float forward[3], right[3], up[3];
    float fov;      /* radians */
    float dist;     /* 0.5 / tan(fov/2) */
} bk_plate;

/* What LUA_load_lens reads back from the script's globals (fisheye.c:1684-1747). */
typedef struct {
    int    map_type;             /* BK_MAP_* after the `map` override */
    int    has_inverse, has_forward;
    int    max_fov, max_vfov;    /* 0 when absent */
    double lens_width, lens_height;   /* 0 when absent */
    char   onload[128];          /* "" when absent or not a string (fisheye.c:1087-1102) */
} bk_lens_info;

/* ---- lifecycle -------------------------------------------------------------------
 * replaces: the three malloc blocks and static state of fisheye.c (306-528, 712-727),
 * init_lua / lua_close (fisheye.c:1222-1265, 678-681). */
bk_ctx     *bk_create(int device);            /* -1: current HIP device; BK_DEVICE_NONE: no device at all */
void        bk_destroy(bk_ctx *ctx);
const char *bk_last_error(const bk_ctx *ctx); /* ctx may be NULL: error of the last failed bk_create */
int         bk_set_stream(bk_ctx *ctx, void *hip_stream);   /* hipStream_t; NULL = default stream */
int         bk_synchronize(bk_ctx *ctx);

/* ---- scripts (the Lua callback surface) -----------------------------------------
 * replaces: LUA_load_globe (fisheye.c:1752-1875) and LUA_load_lens (1659-1750);
 * `src` is the text of <basedir>/lua-scripts/{globes,lenses}/<name>.lua.
 * One interpreter state lives in the context, so script globals leak between
 * loads exactly as in the reference (only the names of fisheye.c:1880-1903 are cleared).
 * The language: what runs while a script LOADS (the chunk, what it calls) is Lua 5.2 (closures, varargs, metatables, goto, coroutines,
 * the string library with patterns, table.*, math.*, bit32.*, os.*, io.*, pcall / xpcall / error, load / dofile / require with
 * package.path / package.preload relative to the working directory; r6: coroutines, the rest of os / io, _G as a proxy of the globals;
 * not provided: string.dump, os.exit - an error the script can see -, and of the debug library what needs a register stack
 * (getlocal / setlocal answer nil, hooks are accepted and never fire; traceback, getinfo, get/setmetatable, get/setupvalue,
 * upvalueid / upvaluejoin and getregistry work); a coroutine created
 * while loading is nil inside the per-pixel callbacks: the build evaluates them on copies of the script state, and a coroutine is a
 * native stack of the original).  What the per-pixel CALLBACKS (lens_inverse, lens_forward,
 * globe_plate and everything they call) may use is narrower - they become GPU code at bk_build: numbers, booleans, nil, string
 * constants, local tables (arrays, records {x = ..}, matrices {{..}, {..}}), constant tables of the chunk, every control structure but goto, the math library, functions
 * defined inside a callback, functions and constant tables passed as arguments, methods of constant objects, varargs.  A script whose
 * callbacks go beyond that (recursion, tables made at run time, functions as values, strings) is NOT refused: bk_build evaluates
 * them with the library's own interpreter on the host instead - seconds instead of milliseconds at 4K - and bk_last_build_path
 * names the construct that forced it (fisheye.c:1551, 1597, 1640 lua_call whatever the script defines). */
int bk_load_globe(bk_ctx *ctx, const char *src, size_t len, const char *chunkname);
int bk_load_lens(bk_ctx *ctx, const char *src, size_t len, const char *chunkname);
int bk_clear_lens(bk_ctx *ctx);    /* lens.valid = false ("not a valid lens", fisheye.c:1080-1083) */
int bk_clear_globe(bk_ctx *ctx);   /* globe.valid = false (fisheye.c:1157-1160) */
int bk_get_lens_info(const bk_ctx *ctx, bk_lens_info *out);
int bk_get_globe(const bk_ctx *ctx, bk_plate plates[BK_MAX_PLATES], int *numplates);
/* bypass the script for the globe (plates already in LUA_load_globe's float form).  The call replaces the plates and drops a globe
 * script's globe_plate function (plates are then chosen by the dot product, fisheye.c:1572-1590); the next bk_build generates its
 * kernels for that.  It runs no script code and leaves the script state alone: the script global `numplates` is set by bk_load_lens,
 * so a lens whose CHUNK reads it (lenses/debug.lua lays its grid out from it) keeps the layout of the plate count it was loaded
 * under until the caller loads it again, as the reference does after every f_globe (fisheye.c:730-741).  plate_to_ray and every per-pixel
 * callback see the new plates at once. */
int bk_set_globe_plates(bk_ctx *ctx, const bk_plate *plates, int numplates);

/* ---- geometry / parameters ------------------------------------------------------
 * bk_resize  replaces F_RenderView's size-change block (fisheye.c:704-727): ps = min(W,H),
 *            (re)allocates globe[6*ps*ps], lensmap[W*H], tints[W*H] in HBM.
 * bk_set_rows restricts this context to output rows [row0,row1) (multi-GPU stripes);
 *            the lensmap, tints and frames it holds cover only those rows.
 * bk_set_frames sizes the resident globe ring: nframes globes of 6*ps*ps bytes. */
int bk_resize(bk_ctx *ctx, int width, int height);
int bk_set_rows(bk_ctx *ctx, int row0, int row1);
int bk_set_frames(bk_ctx *ctx, int nframes);
int bk_set_zoom(bk_ctx *ctx, int zoom_type, int fov_degrees);                       /* cmd_fov/vfov/cover/contain, fisheye.c:955-965,1032-1058 */
int bk_set_rubixgrid(bk_ctx *ctx, int numcells, double cell_size, double pad_size); /* cmd_rubixgrid, fisheye.c:939-953 */

/* ---- lensmap build ----------------------------------------------------------------
 * replaces: create_lensmap (fisheye.c:2367-2397) = calc_zoom + resume_lensmap_inverse
 * (2084-2124) or resume_lensmap_forward (2126-2217), run to completion on the GPU,
 * including the NULL/255 clears of F_RenderView (731-732).
 * display_out (nullable) receives globe.plates[i].display; scale_out lens.scale.
 * A lens_inverse that returns a MALFORMED RESULT (status -1, fisheye.c:1565-1584) ends the reference's scan at that pixel and keeps
 * what it had set by then (2113-2115; rows from the bottom up, pixels left to right): bk_build returns BK_E_SCRIPT with exactly
 * that table in place - the entries the reference's scan had not reached are NULL - and the display flags of what is left.
 * (Stripes: a context knows only its rows; bk_multi_build hands every stripe the group's first failing pixel, a bk_comm host
 * does the same with bk_last_build_bad_key (max over the ranks) and bk_truncate_build.)  Any other run-time failure (arithmetic
 * on nil, a runaway loop - Lua errors the reference's unprotected lua_call does not survive; a malformed lens_forward result)
 * returns BK_E_SCRIPT and leaves an EMPTY lensmap.
 * Script globals (and locals of the script's chunk) that lens_inverse / lens_forward / globe_plate ASSIGN are per-pixel state
 * on the GPU, initialised from their value after the chunk ran: the reference's result for scratch variables and for caches
 * keyed by one of the callback's parameters (`if y ~= lasty then maxx = ..; lasty = y end`: eckert4.lua) - every bundled script.
 * A script that really carries state from one pixel to the next (a counter, a running sum) would not behave as in the reference's
 * sequential scan (fisheye.c:2084-2124), so by DEFAULT (bk_set_sequential_build mode 1) an inverse-map lens whose callbacks read
 * a script global before assigning it outside such a keyed cache, or assign a chunk local at all (bk_lens_carries_state), is built
 * as ONE sequential scan on the host, in the reference's order, by the compiled host module (else the script interpreter):
 * seconds instead of milliseconds at 4K, the reference's result for any script.  (r6) A FORWARD-map lens that carries state is
 * scanned on the host too, by the interpreter, in the reference's own call order (fisheye.c:2126-2217: per plate the last row's
 * lower corners, then row by row from the last up the upper corners left to right and the texels' globe_plate calls).
 * mode 2 = every lens; 0 = never (the GPU build whatever the script does, unless the emitter declines it: bk_last_build_path).
 * Memory: a FORWARD-map build (lenses with lens_forward only) keeps its scratch - screen coordinates of every texel corner and two
 * key planes, about 10 bytes per plate texel + 8 per pixel: 320 MB at 3840x2160 on a cube globe - in the context from one build to
 * the next (allocating it cost more than the build's kernels); it is released when the context builds an inverse map or is destroyed. */
int bk_build(bk_ctx *ctx, int display_out[BK_MAX_PLATES], double *scale_out);
/* how the last bk_build evaluated the lens callbacks: 0 = the GPU kernels; 1 = the interpreter on the host's worker pool (the
 * emitter declined a construct and the callbacks carry no state: every worker has its own copy of the script state); 2 = ONE
 * sequential scan on the host in the reference's order (state carried from call to call, or bk_set_sequential_build 2) - inverse
 * maps: fisheye.c:2084-2124; forward maps: 2126-2217, the corners' and texels' calls in the reference's own sequence.  `why`
 * (nullable) receives the construct the emitter declined and the state finding. */
int bk_last_build_path(const bk_ctx *ctx, char *why /* nullable */, size_t cap);
int bk_set_sequential_build(bk_ctx *ctx, int mode);
int bk_lens_carries_state(bk_ctx *ctx, char *global_name /* nullable */, size_t cap);
/* after a bk_build that returned BK_E_SCRIPT for a malformed result: 1 + scan key (ly * W + (W - 1 - lx)) of the first failing
 * pixel in the reference's scan order, 0 if none; bk_truncate_build NULLs everything the reference's scan would not have reached
 * before the pixel with that key (a no-op for key 0) and recounts display_out (nullable) */
unsigned int bk_last_build_bad_key(const bk_ctx *ctx);
int bk_truncate_build(bk_ctx *ctx, unsigned int bad_key, int display_out[BK_MAX_PLATES]);
int bk_calc_zoom(bk_ctx *ctx, double *scale_out);                                   /* calc_zoom only */
/* Lens modules are compiled with hiprtc on first use (0.2-1.1 s per lens) and kept (a) in the process and (b) on disk:
 * bk_set_cache_dir(dir) / $BLINKY_HIP_CACHE / $XDG_CACHE_HOME/blinky_hip / $HOME/.cache/blinky_hip, in that order
 * ("" or "off" disables the disk cache); a code object is keyed by generated source, embedded headers, GPU arch and
 * library version.  With bk_set_async_compile(ctx, 1) a bk_build that would have to wait for hiprtc starts the
 * compilation on another thread, returns BK_PENDING and leaves the previous lensmap (and display flags) in place,
 * so a render loop keeps drawing - the reference's time-sliced builder never stalls the game either
 * (fisheye.c:2084-2217) - and calls bk_build again on a later frame. */
int bk_set_cache_dir(const char *dir);        /* process-wide; NULL returns to the environment / default location */
int bk_set_async_compile(bk_ctx *ctx, int on);
/* Exactness bookkeeping of the last bk_build.  The kernels evaluate the scripts' transcendentals with a portable
 * libm; the reference's Lua VM calls the platform's.  Every value on the device carries a bound on that
 * discrepancy, and each pixel / texel corner whose DISCRETE outcome (a float narrowing, a comparison, a floor)
 * could depend on it is flagged, re-derived by the host interpreter on the platform libm - the evaluator
 * bk_calc_zoom and bk_load_globe already use - and patched before bk_build returns.
 * flagged = entries re-derived on the host, changed = entries whose value differed from the device's. */
int bk_last_build_fixups(const bk_ctx *ctx, int *flagged, int *changed);
/* direct access to the table (lens.pixels / lens.pixel_tints of the owned rows) */
int bk_set_lensmap(bk_ctx *ctx, const uint32_t *offsets, const uint8_t *tints);
int bk_read_lensmap(bk_ctx *ctx, uint32_t *offsets, uint8_t *tints);
/* The SUB-TEXEL plane (no counterpart in the reference, which keeps (int)(u * platesize), fisheye.c:1988, of the plate position it
 * computes at :2055-2062, and so can only ever show one nearest texel): uint16 [rows][W] beside the lensmap, owned rows only, as the
 * tints are.  For a mapped entry of an inverse map, with U = u * platesize and px = (int)U: qx = (int)((U - px) * 256), 0..255, qy
 * likewise, sub = qx | qy << 8 - exact and reproducible: from the narrowed float ray on, host and device perform the same IEEE
 * operations, U - px is exact and so is * 256; entries the host re-derives (bk_last_build_fixups) have their sub re-derived too
 * (`changed` keeps counting offsets and tints only).  0x8080, the texel's centre, is the value of every entry that has no position of
 * its own: NULL entries, every entry of a FORWARD map (the quad rasteriser has no per-pixel uv), every entry after bk_set_lensmap,
 * entries NULLed by bk_truncate_build, the empty map a failed build leaves.
 * bk_set_subtexel(ctx, 1) opts in (default 0: no plane is allocated, the build kernel stores nothing, every existing path, count and
 * timing is as it was).  On: every later bk_build fills the plane, whichever path it takes (GPU kernels, host worker pool,
 * sequential scan), and bk_set_lensmap resets it to centres.  The plane lives and dies with the lensmap: gone after bk_resize /
 * bk_set_rows, left as it was by a bk_build that returns BK_PENDING.  Switching on over a lensmap already in place conjures no
 * plane: it is absent until the next bk_build, bk_set_lensmap or bk_set_lensmap_subtexel.  Switching off frees it.
 * bk_read_subtexel copies the plane out; bk_set_lensmap_subtexel replaces it (call it after bk_set_lensmap).  BK_E_STATE from either
 * without a lensmap or with the switch off, and from bk_read_subtexel while the plane is absent.
 * Memory: 2 bytes per pixel of the owned rows (16.6 MB at 3840x2160).  Reader: bk_apply_rgba_fb_bilinear_device. */
int bk_set_subtexel(bk_ctx *ctx, int on);
int bk_read_subtexel(bk_ctx *ctx, uint16_t *out);
int bk_set_lensmap_subtexel(bk_ctx *ctx, const uint16_t *sub);

/* ---- globe plates -------------------------------------------------------------------
 * bk_upload_plate replaces render_plate's row memcpy loop (fisheye.c:2441-2449):
 * ps rows of ps bytes from src (pitch src_pitch) into plate `plate` of globe `frame`. */
int   bk_upload_plate(bk_ctx *ctx, int frame, int plate, const uint8_t *src, int src_pitch);
/* the same, pipelined: the rows are copied into a pinned staging buffer (render_plate's memcpy) and the DMA and the
 * re-tiling are only enqueued on the context's stream, so that the caller renders the next plate meanwhile; src may be
 * reused as soon as the call returns.  Three staging slots: the call waits only for the upload three calls ago. */
int   bk_upload_plate_async(bk_ctx *ctx, int frame, int plate, const uint8_t *src, int src_pitch);
/* the way back (the plate copy cmd_saveglobe reads, fisheye.c:1396-1465): ps rows of ps bytes to dst_host */
int   bk_download_plate(bk_ctx *ctx, int frame, int plate, uint8_t *dst_host, int dst_pitch);
/* the plate image f_saveglobe encodes (WritePCXplate's pixel loop, fisheye.c:1438-1456): texel, or 0xFE where
 * the ray through the texel belongs to another plate (ray_to_plate_index / the globe's globe_plate) unless
 * with_margins.  Computed on the device; PCX packing is the caller's (blinky_amd/host/fisheye_hip.c). */
int   bk_save_plate(bk_ctx *ctx, int frame, int plate, int with_margins, uint8_t *dst_host, int dst_pitch);
/* Device layout of a globe frame: 6 plates of bk_globe_pitch() = round_up(ps,64) by bk_globe_rows() =
 * round_up(ps,8) texels, each stored as 16x8-texel tiles of 128 bytes (tiles row-major, rows of a tile
 * 16 bytes apart): a 128-byte line covers a compact patch, so the slanted footprints of the warp touch
 * about half as many lines as with row-major plates.  bk_globe_texel_offset gives the byte offset of a
 * texel inside a frame (0xFFFFFFFF if out of range) for callers that fill plates on the device themselves.
 * Lensmap entries cross this ABI in the reference layout (plate*ps*ps + py*ps + px); the library converts. */
void    *bk_globe_device_ptr(bk_ctx *ctx, int frame);   /* device address of globe `frame` (6*pitch*rows bytes) */
int      bk_globe_pitch(const bk_ctx *ctx);
int      bk_globe_rows(const bk_ctx *ctx);
uint32_t bk_globe_texel_offset(const bk_ctx *ctx, int plate, int px, int py);
/* synthetic plates: the SURVEY.md 8(d) LCG stream generated on the device */
int   bk_fill_plate_lcg(bk_ctx *ctx, int frame, int plate, uint32_t seed_frame);
/* TRUECOLOUR plates (no counterpart in the reference, whose plates are 8-bit; its README names GPU projection of plates captured in
 * frame buffers as its future).  Truecolour globe g = ring slots 4g .. 4g+3 (bk_set_frames(4 * globes)); slot 4g+c holds byte c of
 * every texel, in the tiled layout every slot has - so bk_fill_plate_lcg, bk_download_plate, bk_globe_device_ptr and
 * bk_globe_texel_offset work per byte plane exactly as documented above.  The bytes are opaque: RGBA, BGRA or any other 4-byte
 * texel.  src: ps rows of ps 32-bit texels, rows src_pitch_bytes (>= 4 * ps) apart.
 * bk_upload_plate_rgba         src is host memory; synchronous with respect to src.  The plate travels through a device staging
 *                              buffer of 4*ps*ps bytes, allocated on first use and freed with the context.
 * bk_upload_plate_rgba_device  src is device memory (a renderer's frame buffer, best 16-byte aligned with a pitch that is a
 *                              multiple of 16); the de-interleaving kernel is only enqueued on the context's stream: whatever wrote
 *                              src must be ordered before it on that stream (or complete), and src stay untouched until it has run.
 * Both end a resident session first, as every device entry point but the 8-bit plate uploads. */
int   bk_upload_plate_rgba(bk_ctx *ctx, int globe, int plate, const uint8_t *src_host, int src_pitch_bytes);
int   bk_upload_plate_rgba_device(bk_ctx *ctx, int globe, int plate, const void *src_dev, int src_pitch_bytes);
/* The lensmap's FOOTPRINT (no counterpart in the reference beyond `display`: globe.plates[i].display, fisheye.c:1976, exists so that
 * plates the lens never looks at are not rendered - this is the same question asked per 16x8-texel tile, one 128-byte line of a slot).
 * bk_plate_footprint: which part of plate `plate` the current lensmap (owned rows, bk_set_rows) reads.  rect = {x0, y0, x1, y1} in
 * texels, half-open, tile-granular (x0 / x1 multiples of 16, y0 / y1 of 8, x1 and y1 clipped to ps): the bounding box of the tiles read;
 * all 0 when nothing is read.  *ntiles (nullable) = tiles read.  tiles (nullable): [bk_globe_rows()/8][bk_globe_pitch()/16] bytes,
 * 1 = read; padding tiles (past ps) are never 1.  ntiles > 0 exactly when bk_build's display flag is set for these rows.  Tints play
 * no part.  Computed on the device on the first query (or footprint upload) after the lensmap or the owned rows changed - one pass over
 * the lensmap, one host synchronisation - and kept until they change again: bk_build, bk_set_lensmap, bk_truncate_build, bk_resize,
 * bk_set_rows (a bk_build that returns BK_PENDING changes nothing).  bk_build itself never computes it.  BK_E_STATE without a lensmap.
 * A renderer scissors or culls with rect; a stripe context gets the footprint of its own rows.
 * bk_upload_plate_rgba_footprint / _device: bk_upload_plate_rgba / bk_upload_plate_rgba_device in arguments, ordering, alignment
 * classes (16 / 4 / 1-byte src and pitch), errors and the resident session they end - but ONLY the tiles of the footprint are written
 * (whole tiles, into all four byte planes); every other byte of the four slots keeps its value.  SOURCE TEXELS OUTSIDE rect ARE NEVER
 * READ - neither by the kernel nor, in the host form, by the copy (only rect travels, through the same staging buffer) - so a renderer
 * that scissored to rect may leave the rest of src unwritten.  A plate with an empty footprint is BK_OK and launches nothing.
 * BK_E_STATE without a lensmap.
 * THE CONTRACT: a globe uploaded through the footprint is complete for the lensmap (and owned rows) it was uploaded under, and for
 * nothing else.  After a lensmap change upload again before the next apply - a live renderer uploads every frame anyway.
 * bk_download_plate shows stale tiles outside the footprint.  Every bk_apply* reads such a globe exactly as it reads a fully
 * uploaded one (measured: profiles/rgba_footprint_upload.txt). */
int   bk_plate_footprint(bk_ctx *ctx, int plate, int rect[4], int *ntiles, uint8_t *tiles);
int   bk_upload_plate_rgba_footprint_device(bk_ctx *ctx, int globe, int plate, const void *src_dev, int src_pitch_bytes);
int   bk_upload_plate_rgba_footprint(bk_ctx *ctx, int globe, int plate, const uint8_t *src_host, int src_pitch_bytes);

/* ---- lensmap apply ------------------------------------------------------------------
 * replaces: render_lensmap (fisheye.c:2406-2424).  Unmapped pixels leave dst untouched.
 * pal (nullable unless rubix_on): the 6 tint LUTs of create_palmap (fisheye.c:857-908).
 * bk_apply        dst is host memory (vid.buffer), pitch vid.rowbytes, origin scr_vrect.{x,y};
 *                 it is synchronous.  Only the owned rows are touched.
 * bk_apply_device dst is device memory holding nframes frames of frame_stride bytes each;
 *                 frame f is warped from globe (frame0+f) % nframes_resident.  Asynchronous on the stream.
 *                 dst addresses pixel (0,0) of frame 0 of the WHOLE view; only the owned rows
 *                 [row0,row1) (bk_set_rows) are written, at dst + f*frame_stride + y*pitch + x.  A caller that
 *                 keeps just its stripe (frame_stride = rows*pitch) passes stripe_base - row0*pitch. */
int bk_apply(bk_ctx *ctx, int frame, uint8_t *dst, int dst_pitch, int x0, int y0,
             int rubix_on, const uint8_t pal[BK_MAX_PLATES][256]);
/* bk_apply in two halves: begin enqueues the warp (and the frame's way to pinned host memory) and returns; end waits and
 * delivers into dst exactly as bk_apply does.  Lets a host overlap the GPU's part with its own work, and is how
 * bk_multi_apply keeps several devices busy from one thread. */
int bk_apply_begin(bk_ctx *ctx, int frame, int rubix_on, const uint8_t pal[BK_MAX_PLATES][256]);
int bk_apply_end(bk_ctx *ctx, uint8_t *dst, int dst_pitch, int x0, int y0);
int bk_apply_device(bk_ctx *ctx, int frame0, int nframes, void *dst_dev, int dst_pitch,
                    size_t frame_stride, int x0, int y0, int rubix_on,
                    const uint8_t pal[BK_MAX_PLATES][256]);
/* bk_apply_rgba_device: render_lensmap for TRUECOLOUR globes (bk_upload_plate_rgba*) - the same gather, four bytes per pixel.
 * dst is device memory holding nframes frames of 32-bit pixels, frame_stride bytes apart; frame f is warped from truecolour globe
 * (globe0 + f) % (resident slots / 4) and pixel (x, y) lands at dst + f*frame_stride + (y0+y)*dst_pitch + 4*(x0+x): x0 / y0 are in
 * pixels, dst addresses pixel (0,0) of the WHOLE view, only the owned rows (bk_set_rows) are written and unmapped pixels are left
 * untouched.  Asynchronous on the context's stream; a resident session is ended first, as by bk_apply_device.  One launch of the
 * staged apply's block map (compiled and tuned as for 4 * nframes 8-bit frames): per frame the four byte planes are gathered through
 * it and stored as whole pixels: the traffic of four 8-bit frames and, measured, their time (16 truecolour 3840x2160 frames against one
 * 64-frame bk_apply_device launch over the same slots: 224.6 / 224.4 us cube/panini, 426.0 / 431.5 us cube/hammer; profiles/rgba_apply.txt).
 * Alignment: dst, dst_pitch and frame_stride must be multiples of 4 bytes; make dst + 4 * x0, dst_pitch and frame_stride multiples
 * of 16 - then fully mapped tiles leave as 16-byte stores that fill whole 128-byte lines; otherwise every pixel is a store of its own.
 * BK_E_INVALID: dst_pitch < 4 * (W + x0), a negative origin, globe0 or nframes < 1, or dst / dst_pitch / frame_stride not a multiple
 * of 4.  BK_E_STATE: no lensmap; fewer than 4 ring slots; bk_set_apply_variant(0) (the staged variant only, as for the resident
 * apply); a BK_DEVICE_NONE context.
 * Rubix tints on truecolour frames: bk_apply_rgba_tinted_device below.
 * Out of scope: the resident kernel; a host-pointer bk_apply_rgba; the bk_comm_* / bk_multi_*
 * exchanges, whose stripe buffers are W bytes per row (stripe CONTEXTS - bk_set_rows - do work); the drop-in fisheye_hip.c, whose
 * engine is 8-bit; texel filtering: every pixel is one nearest texel - antialiased frames are bk_apply_rgba_ss2_device below. */
int bk_apply_rgba_device(bk_ctx *ctx, int globe0, int nframes, void *dst_dev, int dst_pitch,
                         size_t frame_stride, int x0, int y0);
/* bk_apply_rgba_tinted_device: f_rubix on truecolour frames.  The reference tints a plate's palette (create_palmap, fisheye.c:857-908:
 * a per-channel blend, fisheye.c:895-901, then the closest palette index) and render_lensmap sends a pixel whose tint is a plate's
 * number through that plate's palette (fisheye.c:2406-2424).  A truecolour texel has no palette to be quantised to: the blend itself is
 * a byte -> byte table per (byte of the texel, plate), and that is what this call takes.  It is bk_apply_rgba_device in every respect -
 * addressing, alignment, owned rows, untouched unmapped pixels, asynchronous on the context's stream, ending a resident session, the
 * same BK_E_INVALID / BK_E_STATE cases - except that byte c of a mapped pixel whose tint t (lens.pixel_tints, fisheye.c:432-449) is
 * below BK_MAX_PLATES is stored as lut[c][t][v] instead of v; tints of 255 and every other value >= BK_MAX_PLATES leave the texel as it
 * is, as in the 8-bit rubix apply.  lut == NULL is BK_E_INVALID.  The tables are generic: per-plate grading or gamma are the same call;
 * bk_create_tintmap_rgba makes the reference's.  The device copy of the 6144 bytes is kept while the bytes and the stream stay the
 * same; it is apart from the 8-bit palette's, so 8-bit rubix launches and truecolour ones alternate without uploads.
 * The launch runs over the TINTED block map (both flavours are kept: alternating with plain launches swaps, it does not recompile).
 * Out of scope: the resident kernel; a host-pointer call; the bk_comm_* / bk_multi_* exchanges; the drop-in fisheye_hip.c; texel
 * filtering (one nearest texel per pixel; bk_apply_rgba_ss2_device below supersamples tinted frames too); tints of different strength per pixel - beyond what a caller's own tables express. */
int bk_apply_rgba_tinted_device(bk_ctx *ctx, int globe0, int nframes, void *dst_dev, int dst_pitch,
                                size_t frame_stride, int x0, int y0, const uint8_t lut[4][BK_MAX_PLATES][256]);
/* bk_apply_rgba_ss2_device: antialiased truecolour frames by 2x2 SUPERSAMPLING, fused into the apply.  The context is sized, built and
 * filled exactly as for bk_apply_rgba_device, at the SUPERSAMPLED size W x H - this is supersampling of the whole pipeline, the
 * renderer's plates included: they are min(W, H) texels - and the call writes frames of Wo = (W + 1) / 2 by Ho = (H + 1) / 2 32-bit
 * pixels: what bk_apply_rgba_device (lut == NULL) or bk_apply_rgba_tinted_device (lut != NULL) would write into a W x H frame,
 * averaged over 2x2 quads with a box filter, without that frame ever being stored.
 * Semantics (exact, integer): for output pixel (X, Y) of frame f let S be the samples (2X+i, 2Y+j), i, j in {0, 1}, that lie inside
 * W x H and whose lensmap entry is not NULL, and n = |S|.  n == 0: the pixel is left untouched.  n > 0: byte c is
 * (sum over S of v_c(s) + n/2) / n in integer arithmetic (n/2 = 0, 1, 1, 2), v_c(s) being the byte the full-size call would store for
 * sample s; a tint is applied per sample, before the average.  All four bytes are treated alike - they are opaque, as everywhere here.
 * Addressing: output pixel (X, Y) of frame f lands at dst + f*frame_stride + (y0+Y)*dst_pitch + 4*(x0+X), frame f warped from
 * truecolour globe (globe0 + f) % (resident slots / 4); dst_pitch, frame_stride, x0, y0 are the half-size frames'.  A context that owns
 * rows [row0, row1) (bk_set_rows) writes output rows [row0/2, (row1+1)/2): row0 must be even and row1 even or H - a quad must not
 * straddle two contexts - otherwise BK_E_STATE.
 * Alignment: as bk_apply_rgba_device (multiples of 4 required); with dst + 4 * x0, dst_pitch and frame_stride multiples of 16 fully
 * mapped tiles leave as 8- or 16-byte stores that fill whole 128-byte lines.  BK_E_INVALID / BK_E_STATE: the cases of
 * bk_apply_rgba_device with Wo in the pitch test, dst_pitch >= 4 * (Wo + x0).  Asynchronous on the context's stream; ends a resident
 * session.  The launch is bk_apply_rgba_device's / bk_apply_rgba_tinted_device's in everything but the kernel - same block maps, same
 * tuning, same LUT copy - so alternating with them or with 8-bit launches swaps and recompiles nothing more than they do among themselves.
 * It reads what the full-size launch reads and stores a quarter of its bytes (measured: profiles/rgba_ss2_apply.txt).
 * Out of scope: the resident kernel; a host-pointer call; the bk_comm_* / bk_multi_* exchanges; factors other than 2; filters other than
 * the box (bilinear texel filtering would need fractional texel coordinates from the lens build). */
int bk_apply_rgba_ss2_device(bk_ctx *ctx, int globe0, int nframes, void *dst_dev, int dst_pitch,
                             size_t frame_stride, int x0, int y0,
                             const uint8_t lut[4][BK_MAX_PLATES][256] /* nullable: NULL = plain, else tinted */);
/* bk_apply_rgba_fb_device: ONE truecolour frame warped straight out of the renderer's six frame buffers - no upload into byte planes,
 * no ring slot, no block map.  For the host the footprint upload was built for: fresh 32-bit plates every frame, one warped frame back.
 * Source: plates_dev[p] is the address of texel (0, 0) of plate p in device memory, a plate ps rows of ps 32-bit texels, rows
 * plate_pitch_bytes[p] apart.  The bytes are opaque, as everywhere in the truecolour API.  An address and its pitch must be multiples
 * of 4 and the pitch at least 4 * ps, otherwise BK_E_INVALID; multiples of 16 are the recommended class (a renderer's frame buffer,
 * as for bk_upload_plate_rgba_device).  Plates may share one allocation (an atlas) or have six different pitches.
 * NULL plates: a plate whose footprint is empty - bk_plate_footprint's ntiles == 0, equivalently bk_build's display flag clear for
 * the owned rows - may be NULL, and its pitch is then ignored; a NULL plate with a non-empty footprint is BK_E_INVALID.  The check
 * uses the cached footprint: the first call after the lensmap or the owned rows changed pays the footprint's one pass over the lensmap
 * and one host synchronisation, every later call nothing.
 * THE CONTRACT ON READS: only texels that some lensmap entry of the owned rows names are read - a subset of the footprint's tiles, so
 * SOURCE TEXELS OUTSIDE rect ARE NEVER READ and a renderer that scissored to bk_plate_footprint's rect is served.  Whatever writes
 * the plates must be ordered before the call on the context's stream (or be complete), and the plates stay untouched until the launch
 * has run.
 * Result: the frame is byte for byte what the existing calls write after bk_upload_plate_rgba_device of the same six plates into a
 * globe - ss2 == 0, lut == NULL: bk_apply_rgba_device(nframes = 1); ss2 == 0, lut given: bk_apply_rgba_tinted_device; ss2 == 1:
 * bk_apply_rgba_ss2_device with the same lut (NULL or given).  Addressing, x0 / y0 in pixels, owned rows only and untouched unmapped
 * pixels are as documented there; tints >= BK_MAX_PLATES leave the texel as it is; ss2 is the exact (sum + n/2) / n over the mapped
 * samples, the tint applied per sample before the average, into the half-size frame of Wo = (W + 1) / 2 pixels a row, and needs row0
 * even and row1 even or H (BK_E_STATE otherwise).  ss2 outside {0, 1} is BK_E_INVALID.
 * Destination: the rules of bk_apply_rgba_device - dst_dev and dst_pitch multiples of 4 required, dst_dev + 4 * x0 and dst_pitch
 * multiples of 16 give 16-byte stores; dst_pitch >= 4 * (W + x0), ss2: 4 * (Wo + x0); a negative origin is BK_E_INVALID.
 * Other errors: BK_E_INVALID for a NULL ctx, plates_dev, plate_pitch_bytes or dst_dev; BK_E_STATE without a lensmap and for a
 * BK_DEVICE_NONE context.  Asynchronous on the context's stream; ends a resident session first, as every other device entry point.
 * It needs no ring slots (bk_set_frames(1) will do), works under bk_set_apply_variant(0) too, and compiles and tunes nothing: it
 * touches neither block map, their tuning state nor the staged launches' LUT copy (its own 6144-byte copy is kept while the bytes and
 * the stream stay the same), so alternating with any other launch recompiles and re-uploads nothing of theirs.
 * Measured at 3840x2160 from plates in HBM (tools/bench_rgba.py --fb, profiles/rgba_fb_apply.txt), against footprint uploads of the
 * displayed plates plus the one-frame bk_apply_rgba_device: cube/panini 38.6 us against 65.2, cube/hammer 61.8 against 117.8; tinted
 * 45.3 / 72.0 and 63.2 / 128.2; ss2 45.1 / 61.0 and 67.8 / 110.6 - and it saves the 112.8 MB of ring a 4K globe takes.  The staged
 * apply ALONE is faster (27.6 and 40.6 us plain): a host whose globes stay resident for many frames stays with bk_apply_rgba_device.
 * Out of scope: more than one frame per call; a host-pointer form; the resident kernel; the bk_comm_* / bk_multi_* exchanges (stripe
 * CONTEXTS - bk_set_rows - do work); the drop-in fisheye_hip.c, whose engine is 8-bit; texel filtering (one nearest texel per sample: bk_apply_rgba_fb_bilinear_device below filters). */
int bk_apply_rgba_fb_device(bk_ctx *ctx, const void *const plates_dev[BK_MAX_PLATES], const int plate_pitch_bytes[BK_MAX_PLATES],
                            void *dst_dev, int dst_pitch, int x0, int y0,
                            const uint8_t lut[4][BK_MAX_PLATES][256] /* nullable: NULL = plain, else tinted */, int ss2);
/* bk_apply_rgba_fb_bilinear_device: bk_apply_rgba_fb_device (ss2 = 0) with BILINEAR texel filtering - the answer to magnification (a
 * fisheye at f_fov 180 stretches the centre plate's texels over several pixels), as ss2 is the answer to minification.  The reference
 * keeps (int)(u * platesize) (fisheye.c:1988) of the position it computes (:2055-2062); the sub-texel plane (bk_set_subtexel above)
 * keeps the next eight bits, and this call blends the four texels around the position.
 * Sources, destination, origin, owned rows, untouched unmapped pixels, alignment classes, NULL plates and errors are those of
 * bk_apply_rgba_fb_device; in addition BK_E_STATE when the context has no sub-texel plane.
 * Semantics per mapped pixel (integer, exact), with (px, py) the entry's texel and sub = qx | qy << 8 - texel centres sit at px + 1/2:
 *     sx = qx + 128;  xa = px - 1 + (sx >> 8);  fx = sx & 255;  xb = xa + 1;  xa, xb clamped to [0, ps - 1]      (ya, yb, fy alike)
 *     per byte c of the texels a00 a01 (row ya), a10 a11 (row yb), all of the entry's OWN plate:
 *         h0 = a00 * (256 - fx) + a01 * fx;  h1 = a10 * (256 - fx) + a11 * fx;  out = (h0 * (256 - fy) + h1 * fy + 32768) >> 16
 * Clamp-to-edge is per plate: filtering ACROSS A CUBE SEAM is out of scope (the last texel row of a plate is repeated, not blended
 * with the neighbouring plate's).  lut given: each of the four texels goes through the pixel's tint (lut[c][t][v], tints >=
 * BK_MAX_PLATES leave it as it is) BEFORE the blend, as ss2 tints per sample before its average.  A constant plate gives that
 * constant; a plane that is 0x8080 everywhere gives bk_apply_rgba_fb_device's frame byte for byte.
 * THE CONTRACT ON READS, restated: texels within ONE TEXEL of a texel some lensmap entry of the owned rows names, clamped to the
 * plate, may be read - also where their weight is 0.  A renderer that scissors to bk_plate_footprint's rect must grow it by one texel
 * on every side, clipped to the plate.
 * Measured: tools/bench_rgba.py --fb --bilinear [--tint], profiles/rgba_fb_bilinear_apply.txt.
 * Out of scope: the staged ring applies (their block map lists exactly the 16-byte chunks a block reads), ss2 combined with the
 * blend, the resident kernel, the bk_comm_* / bk_multi_* exchanges, the drop-in fisheye_hip.c, whose engine is 8-bit. */
int bk_apply_rgba_fb_bilinear_device(bk_ctx *ctx, const void *const plates_dev[BK_MAX_PLATES], const int plate_pitch_bytes[BK_MAX_PLATES],
                                     void *dst_dev, int dst_pitch, int x0, int y0,
                                     const uint8_t lut[4][BK_MAX_PLATES][256] /* nullable: NULL = plain, else tinted */);

/* THE SEAM TABLE: which texel lies one step OUTSIDE each of a plate's four edges - what bk_apply_rgba_fb_bilinear_seams_device blends
 * with at a plate's rim.  Context state of its own, a function of the globe (plates, globe_plate) and the platesize alone: lens, lensmap
 * and owned rows play no part, nor do the rubix grid and tints.
 * Layout: uint32 [6][4][ps + 2] in the reference layout (plate * ps * ps + py * ps + px), 0xFFFFFFFF = "no neighbour: clamp".  For plate p,
 * edge 0 is the row of virtual texels y = -1, edge 1 the row y = ps, edge 2 the column x = -1, edge 3 the column x = ps; index i is the
 * coordinate along the edge + 1, so i = 0 and i = ps + 1 are the corners, each in two edges with the same value.  Plates at or beyond
 * the globe's number are all NULL.
 * Definition, virtual texel (x, y) of plate p: ray = plate_uv_to_ray(p, (x + 0.5) / ps, (y + 0.5) / ps) (fisheye.c:1198);
 * q = ray_to_plate_index(ray) (:2023-2050; a globe_plate callback is evaluated by the library's interpreter on the host, as flagged pixels
 * are); q < 0 or q == p: NULL; else the position on q as the inverse build takes it from the float ray on (:2055-2062, the range test
 * :2065, trunc(u * ps) :1988, the texel test :1971 - a failed test: NULL) and the entry is q * ps * ps + py * ps + px.  Without a callback
 * every step is an IEEE float / double operation.
 * Life: computed on the host on first use (the first seam-aware apply or bk_read_seam_table), uploaded once, kept; bk_build never makes it.
 * Dropped - a caller-set table too - by bk_load_globe, bk_set_globe_plates, bk_clear_globe, bk_load_lens, bk_clear_lens (globe and lens
 * share one interpreter state) and a bk_resize that changes the size; bk_set_rows and bk_build leave it alone.
 * bk_read_seam_table copies out 6 * 4 * (ps + 2) words, computing the table if needed; works on a BK_DEVICE_NONE context; BK_E_STATE
 * without a valid globe or a size.  bk_set_seam_table replaces it (the counterpart of bk_set_lensmap_subtexel: a caller's own adjacency,
 * tests): BK_E_INVALID for an entry that is neither NULL nor below 6 * ps * ps and for a corner whose two copies differ. */
int bk_read_seam_table(bk_ctx *ctx, uint32_t *out);
int bk_set_seam_table(bk_ctx *ctx, const uint32_t *table);
/* bk_apply_rgba_fb_bilinear_seams_device: bk_apply_rgba_fb_bilinear_device that filters across plate seams.  Arguments, sources,
 * destination, alignment classes, origin, owned rows, untouched unmapped pixels and errors are that call's; in addition BK_E_STATE when
 * the seam table cannot be made (no valid globe).
 * Semantics per mapped pixel: xa, xb, ya, yb, fx, fy as there, BEFORE clamping; each of the four positions (xn, yn) is resolved on its own.
 * One inside [0, ps - 1]^2 is the own plate's texel.  One outside takes the seam table's entry E of the pixel's plate for that virtual
 * texel (the corner entry when both coordinates are outside): E NULL, or E's plate passed as a NULL pointer, gives the clamped own-plate
 * texel of bk_apply_rgba_fb_bilinear_device; otherwise the position is texel E.  Blend and rounding are unchanged.  lut given: all four
 * texels go through the PIXEL's tint, wherever they came from.
 * Hence: an all-NULL table gives bk_apply_rgba_fb_bilinear_device's frame byte for byte; a plane of 0x8080 gives
 * bk_apply_rgba_fb_device's frame byte for byte whatever the table holds (weight-0 neighbours are still read); with all six plates given,
 * stripe contexts stitch to the single-context frame.
 * THE CONTRACT ON READS, restated: texels within one texel of a named texel, clamped to the plate, may be read; for a named texel on a
 * plate's first or last row or column, the table's targets of its virtual neighbours may be read too - a renderer that scissors gets
 * the targets from bk_read_seam_table.  A plate with an empty footprint may still be NULL: entries into it clamp.
 * The first call after the table was made, dropped or set (bk_set_seam_table) uploads it: that call allocates, copies from pageable host
 * memory and WAITS for the context's stream - it blocks the host once per table and must not be made during stream capture; make one
 * call before capturing.  Later calls only launch.
 * Measured: tools/bench_rgba.py --fb --bilinear --seams [--tint]. */
int bk_apply_rgba_fb_bilinear_seams_device(bk_ctx *ctx, const void *const plates_dev[BK_MAX_PLATES], const int plate_pitch_bytes[BK_MAX_PLATES],
                                           void *dst_dev, int dst_pitch, int x0, int y0,
                                           const uint8_t lut[4][BK_MAX_PLATES][256] /* nullable: NULL = plain, else tinted */);

/* ---- TRILINEAR: a mip pyramid of the plates and a per-pixel level of detail - the answer to MINIFICATION -----------------------------
 * A whole-globe lens minifies everywhere (a 4K hammer frame: about 2.25 texels a pixel in each direction); nearest and bilinear sampling
 * then keep one texel in five.  bk_apply_rgba_fb_trilinear_device blends two levels of a pyramid of the caller's plates, chosen per
 * pixel by a level-of-detail plane derived from the lensmap and the sub-texel plane.  Everything is integer arithmetic and exact.
 * THE PYRAMID.  Level 0 is the caller's plate, s_0 = ps; s_{k+1} = (s_k + 1) / 2 down to s_{L-1} = 1 (L = 1, 2, 3, 4, 5, 7, 9, 13, 16 for
 * ps = 1, 2, 3, 5, 16, 33, 203, 2160, 26752; at most BK_MIP_MAX_LEVELS).  Texel (x, y) of level k + 1, per byte: (a + b + c + d + 2) >> 2
 * over level k's texels (2x, 2y), (2x + 1, 2y), (2x, 2y + 1), (2x + 1, 2y + 1), coordinates clamped to s_k - 1 (an odd size repeats its
 * last row and column); every level is made from the ROUNDED level below.  Levels 1 .. L - 1 of all six plates live in memory of the
 * context (about a third of 6 * 4 * ps^2 bytes: 37 MB at ps 2160), allocated by the first trilinear apply with mips = 1, freed by a
 * bk_resize that changes the platesize and by bk_destroy; a context that never makes that call allocates nothing.  Making it reads EVERY
 * texel of every non-NULL plate (two launches a frame); a NULL plate's levels stay as they were.
 * bk_mip_info: *levels = L and sizes[k] = s_k for k < L (0 beyond) for the size in place; works without a device; BK_E_STATE without a size.
 * bk_read_mip_level: level 1 <= level < L of `plate` as last made, s_k rows of 4 * s_k bytes dst_pitch apart, into host memory;
 * synchronous.  BK_E_INVALID for a bad plate, level or pitch, BK_E_STATE while there is no pyramid for this platesize.
 * THE LEVEL-OF-DETAIL PLANE: uint16 [row1 - row0][W] beside the lensmap, level << 8 | fraction (in 1/256 level).  For a mapped pixel with
 * texel (px, py) on plate p and sub qx | qy << 8 the position is U = px * 256 + qx, V = py * 256 + qy.  Horizontal step: to the neighbour
 * at x + 1 if that is inside the frame, mapped and on plate p; otherwise to x - 1 under the same test; otherwise none;
 * dh = max(|dU|, |dV|) to that neighbour.  Vertical step dv: the same with y + 1, then y - 1, inside the OWNED rows.  rho = max(dh, dv),
 * 0 with neither step.  rho <= 256: 0; otherwise k = floor(log2 rho) and (k - 8) * 256 + ((rho << 8) >> k) - 256 (the piecewise-linear
 * log2: 257 -> 1, 511 -> 255, 512 -> 256, 768 -> 384).  Then the bias is added (to every mapped pixel's value) and the sum clamped to
 * [0, (L - 1) * 256]; an unmapped pixel has 0.  A forward map's plane of 0x8080 gives differences of texel centres.
 * STRIPES: a stripe context's plane differs from the whole frame's only where a row's vertical neighbour was taken on the other side -
 * the stripe's last row, where that is not the frame's last (its step goes up instead of down).  A halo row is out of scope.
 * bk_set_lod_bias: a signed bias in 1/256 level, default 0; changing it drops the plane.
 * Life: derived on the device by the first trilinear apply or bk_read_lod after the lensmap, the sub-texel plane, the owned rows or the
 * bias changed (bk_build, bk_set_lensmap, bk_set_lensmap_subtexel, bk_set_subtexel, bk_truncate_build, bk_set_rows, bk_resize);
 * never by a build, and not allocated (2 bytes a pixel of the owned rows) before its first use.  bk_set_lensmap_lod replaces it, as
 * bk_set_lensmap_subtexel replaces the sub-texel plane, until one of those events (bk_set_subtexel counts when it CHANGES the switch: setting it
 * to what it is drops nothing); a value above (L - 1) * 256 is BK_E_INVALID.
 * bk_read_lod copies it out, deriving it if needed.  Both answer BK_E_STATE without a lensmap, without a sub-texel plane and on a
 * BK_DEVICE_NONE context. */
#define BK_MIP_MAX_LEVELS 16
int bk_mip_info(bk_ctx *ctx, int *levels, int sizes[BK_MIP_MAX_LEVELS]);
int bk_read_mip_level(bk_ctx *ctx, int plate, int level, void *dst_host, int dst_pitch);
int bk_set_lod_bias(bk_ctx *ctx, int bias);
int bk_read_lod(bk_ctx *ctx, uint16_t *out);
int bk_set_lensmap_lod(bk_ctx *ctx, const uint16_t *lod);
/* bk_apply_rgba_fb_trilinear_device.  Sources, destination, origin, owned rows, untouched unmapped pixels, alignment classes, NULL plates
 * and errors are bk_apply_rgba_fb_bilinear_device's.  mips = 1: the pyramid is made from these plates first, on the same stream;
 * mips = 0: the pyramid as last made is used (BK_E_STATE if there is none for this platesize) - level 0 still comes from the plates
 * given; any other value: BK_E_INVALID.
 * Semantics per mapped pixel, lod its plane value: l = lod >> 8, fl = lod & 255; levels lo = l and hi = min(l + 1, L - 1).  At level k the
 * position is Uk = U >> k, Vk = V >> k (level k's texel j covers level 0's [j * 2^k, (j + 1) * 2^k): the centre convention carries over),
 * and (Uk >> 8, Uk & 255) are what (px, qx) are to bk_apply_rgba_fb_bilinear_device: sx = (Uk & 255) + 128, xa = (Uk >> 8) - 1 + (sx >> 8),
 * fx = sx & 255, xb = xa + 1, both clamped to [0, s_k - 1] of the pixel's OWN plate (rows alike; no seams at any level).  Per byte and
 * level the UNROUNDED v = h0 * (256 - fy) + h1 * fy (h0, h1 as there); out = (v_lo * (256 - fl) + v_hi * fl + 2^23) >> 24 - below 2^32
 * throughout.  At fl = 0 that is (v_lo + 32768) >> 16: a plane of zeros gives bk_apply_rgba_fb_bilinear_device's frame byte for byte
 * (and with subs of 0x8080 bk_apply_rgba_fb_device's); a constant plate gives its constant.  lut given: each of the EIGHT texels goes
 * through the pixel's tint before any blend.
 * Reads: level 0 within one texel of a named texel, clamped, as the bilinear call; pyramid texels of any level; also at weight 0.
 * The first call after the plane's inputs changed derives the plane (one launch, no host wait); the first with mips = 1 for a platesize
 * allocates the pyramid.
 * Measured (tools/bench_rgba.py --fb --trilinear [--tint], profiles/rgba_fb_trilinear_apply.txt; 4K, plates from HBM): the pyramid by itself
 * 65 - 74 us (149.3 MB at 2.03 TB/s on hammer: below the 2.87 TB/s of the footprint re-tile); the frame with mips = 0 against the bilinear
 * call's: hammer 89.4 / 82.0 us, quincuncial 95.1 / 83.0, winkel2 99.5 / 82.9, panini - all of whose pixels blend level 0 with level 1 -
 * 112.0 / 63.2.
 * Out of scope: seams across plates at any level, ss2 combined with it, anisotropic footprints, a pyramid limited to the footprint, a halo
 * row for stripes, the staged ring applies, the resident kernel, the bk_comm_* / bk_multi_* exchanges, the drop-in fisheye_hip.c. */
int bk_apply_rgba_fb_trilinear_device(bk_ctx *ctx, const void *const plates_dev[BK_MAX_PLATES], const int plate_pitch_bytes[BK_MAX_PLATES],
                                      void *dst_dev, int dst_pitch, int x0, int y0,
                                      const uint8_t lut[4][BK_MAX_PLATES][256] /* nullable: NULL = plain, else tinted */, int mips);

/* ---- resident single-frame apply ------------------------------------------------------------------------------------
 * replaces: the per-frame call of render_lensmap (fisheye.c:803 -> 2406-2424) for hosts whose globes stay in device memory.
 * One bk_apply_device launch per frame re-reads the whole block map of the staged apply (2 bytes per pixel and more: half of a
 * 4K frame's traffic) because nothing stays in the caches across a kernel boundary.  bk_apply_resident_begin launches a kernel
 * that STAYS on the device with the block map in its registers; bk_apply_resident_submit hands it one frame - warp globe `frame`
 * into dst_dev (same addressing as bk_apply_device: pixel (0,0) of the whole view, only the owned rows are written, unmapped
 * pixels untouched) - by writing a command into pinned host memory, and returns at once with a ticket; submissions pipeline
 * (up to 32 in flight).  bk_apply_resident_wait(ticket) returns when that frame - and every earlier one - is complete IN
 * MEMORY (any stream, DMA or peer may read it); *gpu_us (nullable) = device time from the kernel seeing the command to the
 * frame's completion.  bk_apply_resident_end makes the kernel leave.
 * Rules: the globe frame and dst of a submission must not be written by anyone else between submit and wait, and whatever
 * produced that globe frame must have COMPLETED (host-synchronised) before the submit - the kernel is not ordered with any
 * stream.  rubix_on / pal are fixed for the session.  The kernel fills the GPU: every other device entry point of this context
 * ends the session first (the next submit starts it again transparently), kernels of other contexts / libraries queue behind
 * it, and a device-wide synchronise blocks until it leaves - which it does by itself after idle_ms (<= 0: 200 ms) without a
 * submission; a later submit relaunches it.  The staged apply variant only. */
int bk_apply_resident_begin(bk_ctx *ctx, int rubix_on, const uint8_t pal[BK_MAX_PLATES][256], double idle_ms);
int bk_apply_resident_submit(bk_ctx *ctx, int frame, void *dst_dev, int dst_pitch, int x0, int y0, uint64_t *ticket);
/* a batch: frame f is warped from globe (frame0 + f) % resident globes into dst_dev + f * frame_stride (bk_apply_device's
 * addressing), one command per frame; blocks only while the command ring is full; *last_ticket = the last frame's */
int bk_apply_resident_submit_batch(bk_ctx *ctx, int frame0, int nframes, void *dst_dev, int dst_pitch, size_t frame_stride,
                                   int x0, int y0, uint64_t *last_ticket);
int bk_apply_resident_wait(bk_ctx *ctx, uint64_t ticket, double *gpu_us);
int bk_apply_resident_end(bk_ctx *ctx);
/* out = {kernel on the device, worker workgroups, blocks per workgroup held in registers, chunk offsets per thread and block,
 * block height, workgroups per CU, kernel launches so far, submissions not yet known complete; of the last session that was ended:
 * min / median / max over its workgroups of the frames a workgroup ran on into the next one without draining; 0} */
int bk_apply_resident_info(bk_ctx *ctx, int out[12]);
/* (r5) The resident kernel beside other work, and under the drop-in calls.
 * bk_set_resident_share: how much of every CU the resident kernel may occupy.  A CU holds up to eight of its workgroups (fewer for the
 * forms that need more registers or LDS); `reserve_slots_per_cu` of those places stay free on every CU - kernels of this context, of
 * other contexts and of other libraries are scheduled there while the kernel is resident, provided they fit what a place leaves
 * (a quarter to an eighth of a CU's registers and LDS) - and the rest is split evenly between `parts` contexts of the same device, of
 * which this one is number `part`: stripe contexts on a one-GPU box each keep their own resident kernel.  A form that fits a CU no more
 * often than the reserve asks to leave free (64 KiB of staging for a scrambled table: twice) keeps one place per context - the reserve
 * yields, such a workgroup leaves most of the CU to others anyway.  Default 0 / 1 / 0: the whole chip.  Takes effect at the next bk_apply_resident_begin / relaunch.  (Measured and not used: a CU-masked stream -
 * hipExtStreamCreateWithCUMask streams are blocking streams, so every null-stream operation of the process, PyTorch's default
 * stream included, then waits for the resident kernel to leave.)
 * bk_set_resident_apply(ctx, 1): the per-frame calls of the drop-in go through the resident kernel - bk_apply / bk_apply_begin .. _end
 * submit the frame as a command, and none of bk_apply* / bk_upload_plate* ends the session.  How plates and frames travel depends on the
 * share: with reserve_slots_per_cu >= 1 (recommended for a drop-in: fisheye_hip.c's default) this context's small kernels run beside
 * the resident kernel, so plates are re-tiled on the device and a fully mapped frame is copied straight into the caller's buffer, as
 * without a resident kernel; with 0 the kernel may hold every place of the chip, and bk_upload_plate / bk_upload_plate_async re-tile
 * the plate on the HOST (render_plate's row memcpy, fisheye.c:2441-2449, writes tiles instead of rows) and move it with one DMA, the
 * frame comes back through a pinned copy + host rows - about 1 ms more host time per 3840x2160 frame, no kernel launch at all per frame
 * (a session is begun by the first bk_apply after a build, with that call's
 * rubix flag and palette, and begun again when they change).  Everything else (bk_build, bk_resize, bk_apply_device ...) still ends it.
 * A process-wide requirement of the resident kernel: the HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues
 * (default 4), and a stream that shares a queue with the resident kernel waits until it idles out.  Loading this library sets the
 * variable to 16 if it is unset (the runtime reads it at its first call); BLINKY_HIP_KEEP_HW_QUEUES=1 prevents that, a value already set
 * is kept, and when the runtime was loaded first the first session prints one line on stderr saying so. */
int bk_set_resident_share(bk_ctx *ctx, int part, int parts, int reserve_slots_per_cu);
int bk_set_resident_apply(bk_ctx *ctx, int on);

/* ---- multi-GPU: row stripes + RCCL over xGMI ---------------------------------------------------------------
 * No counterpart in the reference (fisheye.c is single-threaded CPU code).  Every output pixel is independent, so
 * GPU r of N owns rows [H*r/N, H*(r+1)/N): it builds and keeps only that stripe of the lensmap (no exchange, ever),
 * holds a full replica of the globe, warps its stripe; ONE exchange step reassembles frames.  Stripe buffers are
 * tight: [nframes][rows_r][W] bytes; frame buffers are tight [slots][H][W] with `frame_stride` bytes between slots.
 * An exchange is asynchronous: it starts once the work queued on the context's stream so far (the warp of the stripe)
 * has finished and runs on the communicator's own stream, so that the NEXT batch's warp overlaps the stripes' travel;
 * `slot` (0..BK_COMM_SLOTS-1) names it for bk_comm_wait.  librccl is loaded on first use.
 *
 * bk_comm: ONE rank.  Ranks may be processes (one per GPU, e.g. under torchrun / mpirun: rank 0 calls
 * bk_comm_unique_id and ships the 128 bytes to the others by any means) or several contexts of one process. */
#define BK_COMM_ID_BYTES 128
#define BK_COMM_SLOTS 4     /* exchanges in flight that a caller can tell apart (double / quadruple buffering) */
typedef struct bk_comm bk_comm;
int         bk_comm_unique_id(uint8_t id[BK_COMM_ID_BYTES]);                      /* ncclGetUniqueId */
/* joins the communicator (ncclCommInitRank on the context's device; waits until all nranks joined, at most BLINKY_HIP_COMM_TIMEOUT
 * seconds - default 60 - after which it fails and bk_last_error(NULL) says that a rank never arrived) and restricts the
 * context to this rank's stripe (bk_set_rows); needs bk_resize first.  nranks == 1 needs no id. */
bk_comm    *bk_comm_create(bk_ctx *ctx, int nranks, int rank, const uint8_t id[BK_COMM_ID_BYTES]);
void        bk_comm_destroy(bk_comm *c);
const char *bk_comm_last_error(const bk_comm *c);                                  /* c may be NULL: last failed create */
int         bk_comm_stripe(const bk_comm *c, int rank, int *row0, int *row1);      /* any rank's rows */
int         bk_comm_restripe(bk_comm *c);                                          /* after a later bk_resize */
/* stripes of equal WORK instead of equal height (collective: every rank calls it after a bk_build): what every row costs
 * the apply - for the default (staged) apply the costs of the row's blocks in this rank's block map: globe lines staged,
 * mapped pixels, a constant per block; for the direct-gather variant its mapped pixels - is summed over the ranks
 * (ncclAllReduce), the rows are cut into shares of equal cost (multiples of 8 rows) and this rank's context gets its new
 * stripe (bk_set_rows).  Build again afterwards; bk_comm_stripe tells the new stripes.  For lenses that leave part of the
 * screen unmapped or sample the globe unevenly (hammer's ellipse: with equal heights the ranks that own the top and the
 * bottom of the screen have a fraction of the middle ranks' work).  Every rank must run the same apply variant. */
int         bk_comm_rebalance(bk_comm *c);
/* display[] |= every other rank's (which plates the WHOLE frame reads, fisheye.c:1976): ncclAllReduce(MAX); synchronous */
int         bk_comm_or_display(bk_comm *c, int display[BK_MAX_PLATES]);
/* every frame of the batch onto `root` (what a single display needs): grouped ncclSend / ncclRecv; frames_dev is
 * used on the root only and receives frame f at slot f */
int         bk_comm_gather(bk_comm *c, const void *stripe_dev, int nframes, int root, void *frames_dev, size_t frame_stride, int slot);
/* batches: frame f is reassembled on rank f % N at slot f / N (a gather whose root rotates): all N*(N-1) xGMI links
 * carry stripes at once and every GPU ends up with 1/N of the batch as whole frames */
int         bk_comm_exchange_rotating(bk_comm *c, const void *stripe_dev, int nframes, void *frames_dev, size_t frame_stride, int slot);
/* the context's stream waits - on the device, the host does not block - for the exchange last posted with `slot`:
 * call before warping into the stripe buffer, or reading the frames, that exchange used */
int         bk_comm_wait(bk_comm *c, int slot);
int         bk_comm_synchronize(bk_comm *c);         /* host waits for the context's stream and every posted exchange */

/* bk_multi: N stripe contexts + their communicators driven by ONE host thread - what a single-process C host
 * (blinky_amd/host/fisheye_hip.c) uses to spread F_RenderView's warp over the node's GPUs.  ncclCommInitAll; every
 * exchange is posted for all ranks inside one ncclGroup.  A device named twice (one-GPU box; RCCL refuses duplicates)
 * or BLINKY_HIP_COMM=copy selects device-to-device copies over the same schedule instead. */
typedef struct bk_multi bk_multi;
bk_multi   *bk_create_multi(int ndev, const int *devices);
void        bk_destroy_multi(bk_multi *m);
const char *bk_multi_last_error(const bk_multi *m);
int         bk_multi_size(const bk_multi *m);
bk_ctx     *bk_multi_ctx(bk_multi *m, int i);        /* stripe context i (introspection, per-context calls) */
bk_comm    *bk_multi_comm(bk_multi *m, int i);       /* after bk_multi_resize */
int         bk_multi_uses_rccl(const bk_multi *m);
int         bk_multi_lensmap_valid(const bk_multi *m);   /* 1 when every stripe context holds a lensmap built for its current rows */
/* the per-context calls applied to every stripe context (same meaning as their bk_* namesakes) */
int bk_multi_load_globe(bk_multi *m, const char *src, size_t len, const char *chunkname);
int bk_multi_load_lens(bk_multi *m, const char *src, size_t len, const char *chunkname);
int bk_multi_clear_lens(bk_multi *m);
int bk_multi_clear_globe(bk_multi *m);
int bk_multi_resize(bk_multi *m, int width, int height);          /* + stripes: context i owns rows [H*i/N, H*(i+1)/N) */
int bk_multi_rebalance(bk_multi *m, int *bounds_out /* [N+1], nullable */);   /* bk_comm_rebalance for the group; then bk_multi_build again */
int bk_multi_set_frames(bk_multi *m, int nframes);
int bk_multi_set_zoom(bk_multi *m, int zoom_type, int fov_degrees);
int bk_multi_set_rubixgrid(bk_multi *m, int numcells, double cell_size, double pad_size);
int bk_multi_upload_plate(bk_multi *m, int frame, int plate, const uint8_t *src, int src_pitch);   /* replica on every GPU */
int bk_multi_fill_plate_lcg(bk_multi *m, int frame, int plate, uint32_t seed_frame);
int bk_multi_synchronize(bk_multi *m);       /* host waits for every stream of every rank */
int bk_multi_wait(bk_multi *m, int slot);    /* bk_comm_wait on every rank */
/* all stripes built concurrently (one host thread per device); display_out = OR over the stripes */
int bk_multi_build(bk_multi *m, int display_out[BK_MAX_PLATES], double *scale_out);
/* host frame: every device warps its stripe and copies it straight into dst (N PCIe links side by side) */
/* bk_set_resident_apply on every stripe context; contexts that share a device (a device named twice) split the places of its CUs
 * between them (bk_set_resident_share) so that each keeps its own resident kernel */
int bk_multi_set_resident_apply(bk_multi *m, int on);
int bk_multi_apply(bk_multi *m, int frame, uint8_t *dst, int dst_pitch, int x0, int y0, int rubix_on,
                   const uint8_t pal[BK_MAX_PLATES][256]);
/* device frames: warp into per-device stripe buffers, then gather / rotating exchange as bk_comm_* */
int bk_multi_apply_stripes(bk_multi *m, int frame0, int nframes, void *const *stripes_dev, int rubix_on,
                           const uint8_t pal[BK_MAX_PLATES][256]);
int bk_multi_gather(bk_multi *m, void *const *stripes_dev, int nframes, int root, void *frames_dev, size_t frame_stride, int slot);
int bk_multi_exchange_rotating(bk_multi *m, void *const *stripes_dev, int nframes, void *const *frames_dev, size_t frame_stride, int slot);

/* plain device buffers for hosts that do not link HIP themselves (zero-filled; ordered on the context's stream) */
void *bk_dev_alloc(bk_ctx *ctx, size_t bytes);
void  bk_dev_free(bk_ctx *ctx, void *dev_ptr);
int   bk_dev_read(bk_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);   /* synchronous */

/* rubix palettes: create_palmap / find_closest_pal_index (fisheye.c:835-908); basepal = 768 bytes */
void bk_create_palmap(const uint8_t *basepal, uint8_t pal_out[BK_MAX_PLATES][256]);
/* the same tints for truecolour texels (bk_apply_rgba_tinted_device): create_palmap's blend (fisheye.c:895-901) of the six tint colours
 * (fisheye.c:863-886) at percent = 256/6 (fisheye.c:860), without the palette search that follows it there (fisheye.c:903):
 * lut_out[c][j][v] = clamp(v + ((42 * (tint[j][ch] - v)) >> 8)), ch = channel_of_byte[c]: 0 = red, 1 = green, 2 = blue; any other
 * value (alpha, padding): the identity.  RGBA texels: {0, 1, 2, 3}; BGRA: {2, 1, 0, 3}.  Host code; no context, no device. */
void bk_create_tintmap_rgba(const int channel_of_byte[4], uint8_t lut_out[4][BK_MAX_PLATES][256]);

/* ---- introspection ---------------------------------------------------------------------
 * (developer knobs, ablations, statistics and test hooks - the bk_debug_* entry points - are declared in
 *  include/blinky_hip_debug.h and exist only when the library is built with BK_DEBUG_API, the Makefile's default) */
int         bk_get_size(const bk_ctx *ctx, int *width, int *height, int *platesize, int *row0, int *row1);
const char *bk_version(void);
/* selects the apply kernel: 0 = direct gather, 2 = workgroup-cooperative LDS staging (default) */
int         bk_set_apply_variant(bk_ctx *ctx, int variant);
/* How the staged apply picks its block height (128x8 / 128x16 / 128x32 pixels) after a build: 1 (default) = the candidates
 * its cost model ranks within 20 % of the best are compiled and the caller's own first launch is TIMED on each (about
 * 0.7 ms more per lensmap at 3840x2160, for up to 17 % per frame where the model misses); 0 = the cost model alone. */
int         bk_set_blockmap_tuning(bk_ctx *ctx, int measured);
/* milliseconds of the last bk_build's device work (HIP events on the context stream) */
double      bk_last_build_ms(const bk_ctx *ctx);
/* The entries a build flags (results that hinge on the platform libm's last bits) are re-derived on the host: by the script
 * interpreter, or - when the machine has a C++ compiler - by the generated lens code itself compiled for the host and loaded
 * with dlopen (a fraction of a microsecond per entry instead of 4-10 us).  The compiler ($BLINKY_HIP_HOSTCXX, else c++ / g++ /
 * clang++ on $PATH, else ROCm's clang; "off" = none) runs on another thread, its output is cached beside the device code
 * objects (bk_set_cache_dir); until it is there the interpreter answers - same results either way.
 * bk_set_host_compile(0) switches the mechanism off for the process.  bk_host_module_ready: 1 when the current lens + globe's
 * module is loaded; with wait != 0 it is compiled now if need be. */
int         bk_set_host_compile(int on);
int         bk_host_module_ready(bk_ctx *ctx, int wait);
/* host-side script arithmetic (chunk execution, calc_zoom, globe loading, re-derivation of flagged pixels): 0 = the
 * platform libm, which is what the reference's Lua VM calls (default: scale, lens_width, plates bit-identical to the
 * reference on the same machine); 1 = the portable bkm.h functions the GPU kernels use.  (Values >= 2 select the
 * stand-in libms of the test suite and exist only in builds with the debug API: include/blinky_hip_debug.h.) */
int         bk_set_host_math(bk_ctx *ctx, int portable);
/* text the scripts print()ed since the context was created (the reference sends it to stdout) */
const char *bk_script_console(bk_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
