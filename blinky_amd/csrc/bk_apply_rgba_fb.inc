// bk_apply_rgba_fb.inc -- part of bk_apply_coop.hip: the TRUECOLOUR apply straight from six row-major frame buffers
// (bk_apply_rgba_fb_device) for gfx950.
//
// One frame per call out of plates that are ordinary 32-bit images in device memory: no upload into byte planes, no ring slot, no block
// map, no tuning - the lensmap says which texel every pixel takes, and a pixel is ONE dword load where the staged kernel gathers four
// bytes out of four planes.  The models are apply_direct4 (bk_apply.hip) and rgba_direct_frames (bk_apply_rgba.inc).
//
// Decoding.  The device lensmap holds offsets into the tiled globe (bk_texel_offset); a frame buffer wants (plate, px, py).  No second,
// converted lensmap is kept: the inverse (bk_texel_coords) is taken per pixel, exactly, for every globe bk_resize accepts
// (6 * gp * ph < 2^32 - 1, platesizes up to about 26700):
//     plate = off / (gp * ph)   as five comparisons against multiples of gp * ph (plate < 6; anything beyond counts as plate 5)
//     ty    = tile / tpr        tile = (off % (gp * ph)) >> 7, tpr = gp / 16: an estimate q = __umulhi(tile, M), M = floor(2^32 / tpr),
//                               and ONE correction step: if (tile - q * tpr >= tpr) ++q
// M * tpr = 2^32 - e with 0 <= e < tpr, so tile * M / 2^32 = tile / tpr - tile * e / (tpr * 2^32), and the term taken off is below
// tile / 2^32 < 1 for ANY 32-bit tile: q is the quotient or one less, never more, and the remainder test decides which.  (The estimate
// alone is not enough: without the step, or with M + 1 and no step, layouts from gp = 21184 on decode some tiles a row off.)
// BK_FB_PLATE / BK_FB_TEXEL below are the one statement of it for the kernel and for bk_debug_fb_decode_check, which holds them to
// bk_texel_coords on the CPU - every tile of a plate, every plate's boundaries; tests/test_rgba_fb_abi.py runs it for EVERY padded plate
// width bk_resize accepts, at the largest height it accepts with it.
// The six pointers and pitches travel by value in the kernel arguments (BkFbPlates) and are picked by the same five comparisons
// (BK_FB_PICK: selects - picked by number, an indexed copy of the struct lives in scratch).
//
// Work layout, full size (apply_rgba_fb_kernel<RUBIX>): a workgroup of 256 covers a 128 x 8 patch of the frame - 32 lanes x 4
// consecutive pixels by 8 rows, a wave two rows - so the source lines the patch touches are shared in the CU's L1 and the XCD's L2.
// Per lane: its four lensmap entries (one 16-byte load when W is a multiple of 4, four dword loads otherwise - rows are W entries
// apart), then four dword loads from the plates, all four addresses formed before the first load is used; an unmapped pixel, or one
// past W, re-reads the lane's own first lensmap entry instead (valid, cached, discarded), so no load hangs on a branch.  Default
// cache policy: neighbours share lines.  Store: one non-temporal 16-byte store when all four pixels are mapped, inside W and the
// address is 16-byte aligned; a dword store per mapped pixel otherwise.
// RUBIX: the lane's four tints are a dword (or four bytes) of the tint plane; all four planes' LUTs - 6 KiB, no staging buffer competes
// for the LDS here - are loaded by the workgroup before anything else; four ds_read_u8 per pixel whose tint is below BK_MAX_PLATES.
// SS2 (apply_rgba_fb_ss2_kernel<RUBIX>): a lane owns four OUTPUT pixels = 8 x 2 samples, a workgroup 128 x 8 output pixels; nothing
// crosses lanes.  A sample's dword is split into its even and odd bytes (v & 0x00FF00FF, (v >> 8) & 0x00FF00FF) and summed in 16-bit
// fields, 4 * 255 at most; n = 4: (s + 2) >> 2 on both fields at once, otherwise bk_ss2_avg per field (thirds by 21846 >> 16).
// As built (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any of the four):
//     full size plain / tinted: 23 / 27 VGPRs = 8 waves per SIMD;  ss2 plain / tinted: 47 / 70 VGPRs = 8 / 7 waves per SIMD
// Measured (tools/bench_rgba.py --fb [--tint] [--ss2], profiles/rgba_fb_apply.txt; B + P = footprint uploads + the one-frame staged apply
// of the same plates, D = this launch, 4K, plates from HBM): plain panini D 38.6 us against B + P 65.2, hammer 61.8 / 117.8; tinted
// 45.3 / 72.0 and 63.2 / 128.2; ss2 45.1 / 61.0 and 67.8 / 110.6 - D < B + P by more than both spreads everywhere, and D > P alone
// everywhere (27.6 / 40.6 plain): resident globes stay with the staged apply.  DESIGN.md 3.1 has the table and what is suspected.

struct BkFbPlates {
    const uint8_t *p[BK_MAX_PLATES];
    uint32_t pitch[BK_MAX_PLATES];
};

// floor(2^32 / tpr) (tpr = gp / 16 >= 4)
static inline uint32_t bk_fb_recip(uint32_t tpr) { return (uint32_t)(0x100000000ull / tpr); }

// the plate of a device offset; pb = gp * ph (6 * pb fits 32 bits)
#define BK_FB_PLATE(off, pb)                                                                                                       \
    ((uint32_t)((off) >= (pb)) + (uint32_t)((off) >= 2u * (pb)) + (uint32_t)((off) >= 3u * (pb)) + (uint32_t)((off) >= 4u * (pb)) + \
     (uint32_t)((off) >= 5u * (pb)))
// offset inside a plate -> texel column, texel row; tpr_m = bk_fb_recip(tpr), hi32 = the high half of a 32 x 32 product
#define BK_FB_TEXEL(rem, tpr, tpr_m, hi32, px, py)                                                                                 \
    do {                                                                                                                           \
        const uint32_t rem_ = (rem), tile_ = rem_ >> 7;                                                                            \
        uint32_t ty_ = hi32(tile_, (tpr_m)), tx_ = tile_ - ty_ * (tpr);      /* the quotient or one less (head comment) */            \
        if (tx_ >= (tpr)) { ++ty_; tx_ -= (tpr); }                                                                                 \
        (px) = tx_ * 16u + (rem_ & 15u);                                                                                           \
        (py) = ty_ * 8u + ((rem_ >> 4) & 7u);                                                                                      \
    } while (0)

#if BK_DEBUG_API
static inline uint32_t bk_fb_hi32_host(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
static inline bool bk_fb_decode_differs(uint32_t gp, uint32_t ph, uint32_t tpr_m, uint32_t off)
{
    const uint32_t pb = gp * ph, tpr = gp >> 4;
    uint32_t p0, x0, y0, x1, y1;
    bk_texel_coords(gp, ph, off, &p0, &x0, &y0);
    const uint32_t p1 = BK_FB_PLATE(off, pb);
    BK_FB_TEXEL(off - p1 * pb, tpr, tpr_m, bk_fb_hi32_host, x1, y1);
    return p0 != p1 || x0 != x1 || y0 != y1;
}
// the kernel's decode against bk_texel_coords for a globe whose padded plates are gp x ph: one texel of EVERY 128-byte tile of the last
// plate (the low seven offset bits, which pass through both, vary from tile to tile; what happens inside a plate does not depend on the
// plate, whose offset is taken off first) and, for every plate, its first and last two tiles at both ends of their low bits - where the
// comparisons decide.  -> the number of texels that decode differently, -1 for a layout bk_resize does not accept
extern "C" long long bk_debug_fb_decode_check(int gp, int ph)
{
    if (gp < 64 || (gp & 63) || ph < 8 || (ph & 7) || ph > gp || 6ull * (uint64_t)gp * (uint64_t)ph >= 0xFFFFFFFFull) return -1;
    const uint32_t pb = (uint32_t)gp * (uint32_t)ph, m = bk_fb_recip((uint32_t)gp >> 4);
    long long bad = 0;
    for (uint32_t tile = 0; tile < pb >> 7; ++tile) bad += bk_fb_decode_differs((uint32_t)gp, (uint32_t)ph, m, 5u * pb + tile * 128u + ((tile * 37u) & 127u));
    for (uint32_t p = 0; p < 6; ++p)
        for (uint32_t low : {0u, 127u, 128u, 255u}) {
            bad += bk_fb_decode_differs((uint32_t)gp, (uint32_t)ph, m, p * pb + low);
            bad += bk_fb_decode_differs((uint32_t)gp, (uint32_t)ph, m, p * pb + pb - 256u + low);
        }
    return bad;
}
#endif

struct BkFbGeom {
    uint32_t pb, tpr, tpr_m;      // gp * ph, gp / 16, bk_fb_recip(tpr)
    int W, rows;                  // of the owned rows' lensmap ([rows][W], as d_offsets / d_tints)
    int lmap4;                    // W % 4 == 0: a lane's four entries are one aligned 16-byte load, its four tints one dword
};

// The plate pick, stated once: the plate of device offset `off` (a name or a member: it stands bare below), the plate's base and its
// pitch out of the BkFbPlates `s` and the BkFbGeom `g` of the function it stands in.  BK_FB_PLATE's five comparisons, kept as they
// are: they also pick the pointer and the pitch (selects on the comparisons - picked by the plate's NUMBER the compiler makes an
// indexed copy of the struct in scratch, 80 bytes per lane).
// A macro, as BK_FB_STORE4 and BK_FB_BILINEAR_AT below: a __forceinline__ function with reference or struct results was tried for each
// and is the same arithmetic but not the same kernel - other register allocation in all eight, and in the function forms tried together
// the tinted ss2 kernel at 82 VGPRs for 70.  Expanded in place they are, instruction for instruction, the kernels as they were.
#define BK_FB_PICK(off, plate, base, pitch)                                                                                        \
    const bool c1 = off >= g.pb, c2 = off >= 2u * g.pb, c3 = off >= 3u * g.pb, c4 = off >= 4u * g.pb, c5 = off >= 5u * g.pb;       \
    plate = (uint32_t)c1 + (uint32_t)c2 + (uint32_t)c3 + (uint32_t)c4 + (uint32_t)c5;                                              \
    base = c5 ? s.p[5] : c4 ? s.p[4] : c3 ? s.p[3] : c2 ? s.p[2] : c1 ? s.p[1] : s.p[0];                                           \
    pitch = c5 ? s.pitch[5] : c4 ? s.pitch[4] : c3 ? s.pitch[3] : c2 ? s.pitch[2] : c1 ? s.pitch[1] : s.pitch[0]

// lensmap entry `off` decoded: its plate's number (returned), base and pitch, the texel's column and row
__device__ __forceinline__ uint32_t bk_fb_locate(const BkFbPlates &s, const BkFbGeom &g, uint32_t off, const uint8_t *&base, uint32_t &pitch, uint32_t &px,
                                                 uint32_t &py)
{
    uint32_t plate;
    BK_FB_PICK(off, plate, base, pitch);
    BK_FB_TEXEL(off - plate * g.pb, g.tpr, g.tpr_m, __umulhi, px, py);
    return plate;
}

// where the texel of lensmap entry `off` lies in the caller's plates
__device__ __forceinline__ const uint32_t *bk_fb_texel(const BkFbPlates &s, const BkFbGeom &g, uint32_t off)
{
    const uint8_t *base;
    uint32_t plate, pitch, px, py;
    BK_FB_PICK(off, plate, base, pitch);
    BK_FB_TEXEL(off - plate * g.pb, g.tpr, g.tpr_m, __umulhi, px, py);
    return reinterpret_cast<const uint32_t *>(base + (size_t)py * pitch + (size_t)px * 4u);
}

// byte c of texel v through row t of plane c's LUT (lut_s = uint8 [4][BK_MAX_PLATES][256] in LDS); tints >= BK_MAX_PLATES: as it is
__device__ __forceinline__ uint32_t bk_fb_tint(uint32_t v, uint32_t t, const uint8_t *lut_s)
{
    if (t < (uint32_t)BK_MAX_PLATES) {
        const uint8_t *row = lut_s + t * 256u;
        v = (uint32_t)row[v & 0xFFu] | ((uint32_t)row[BK_PAL_BYTES + ((v >> 8) & 0xFFu)] << 8) |
            ((uint32_t)row[2 * BK_PAL_BYTES + ((v >> 16) & 0xFFu)] << 16) | ((uint32_t)row[3 * BK_PAL_BYTES + (v >> 24)] << 24);
    }
    return v;
}

// N consecutive entries of lensmap row `row` from column x (x % 4 == 0, x < W) and, RUBIX, their tints; entries past W: NULL
template <int N, bool RUBIX>
__device__ __forceinline__ void bk_fb_entries(const uint32_t *__restrict__ lmap, const uint8_t *__restrict__ tints, const BkFbGeom &g, int row, int x,
                                              uint32_t o[N], uint32_t t[N])
{
    const size_t at = (size_t)row * g.W + x;
    if (g.lmap4) {
#pragma unroll
        for (int k = 0; k < N; k += 4) {
            const bool in = x + k < g.W;
            const uint4 q = in ? *reinterpret_cast<const uint4 *>(lmap + at + k) : make_uint4(BK_NULL_OFFSET, BK_NULL_OFFSET, BK_NULL_OFFSET, BK_NULL_OFFSET);
            o[k] = q.x; o[k + 1] = q.y; o[k + 2] = q.z; o[k + 3] = q.w;
            if (RUBIX) {
                const uint32_t t4 = in ? *reinterpret_cast<const uint32_t *>(tints + at + k) : 0xFFFFFFFFu;
                t[k] = t4 & 0xFFu; t[k + 1] = (t4 >> 8) & 0xFFu; t[k + 2] = (t4 >> 16) & 0xFFu; t[k + 3] = t4 >> 24;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const bool in = x + k < g.W;
            o[k] = in ? lmap[at + k] : BK_NULL_OFFSET;
            if (RUBIX) t[k] = in ? (uint32_t)tints[at + k] : 255u;
        }
    }
    if (!RUBIX) (void)t;
}

// the workgroup's LUTs into LDS: 6 KiB = 1536 dwords, six per thread of 256
__device__ __forceinline__ void bk_fb_load_lut(const uint8_t *__restrict__ lut, uint8_t *lut_s)
{
    const uint32_t *src = reinterpret_cast<const uint32_t *>(lut);
    uint32_t *dst = reinterpret_cast<uint32_t *>(lut_s);
    uint32_t w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = src[threadIdx.x + 256 * i];
#pragma unroll
    for (int i = 0; i < 6; ++i) dst[threadIdx.x + 256 * i] = w[i];
    __syncthreads();
}

// a kernel's first statement: the LUTs' place in LDS (16 bytes nobody reads in a plain kernel) and, tinted, the load
#define BK_FB_LUT_S(lut)                                                                                                           \
    __shared__ __attribute__((aligned(16))) uint8_t lut_s[RUBIX ? 4 * BK_PAL_BYTES : 16];                                          \
    if (RUBIX) bk_fb_load_lut(lut, lut_s)

// The store tail: a lane's four pixels v[0..3] to `out`, w0..w3 = pixel k is written: one non-temporal 16-byte store when all four are
// and the address is 16-byte aligned, a dword store per written pixel otherwise.  `all` is w0 && w1 && w2 && w3 as the kernel has it -
// the full-size kernels a flag made after `out`, ss2 the expression itself: which of the two, and where, is part of the code that comes
// out, so each keeps its own.  (A macro for BK_FB_PICK's reason.)
#define BK_FB_STORE4(out, v, all, w0, w1, w2, w3)                                                                                  \
    do {                                                                                                                           \
        if ((all) && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {                                                              \
            typedef uint32_t v4u __attribute__((ext_vector_type(4)));                                                              \
            v4u q_ = {(v)[0], (v)[1], (v)[2], (v)[3]};                                                                             \
            __builtin_nontemporal_store(q_, reinterpret_cast<v4u *>(out));                                                         \
        } else {                                                                                                                   \
            if (w0) reinterpret_cast<uint32_t *>(out)[0] = (v)[0];                                                                 \
            if (w1) reinterpret_cast<uint32_t *>(out)[1] = (v)[1];                                                                 \
            if (w2) reinterpret_cast<uint32_t *>(out)[2] = (v)[2];                                                                 \
            if (w3) reinterpret_cast<uint32_t *>(out)[3] = (v)[3];                                                                 \
        }                                                                                                                          \
    } while (0)

// dst = pixel (0, 0) of the owned rows' part of the frame (origin applied); grid = (ceil(W / 128), ceil(rows / 8))
template <bool RUBIX>
__global__ __launch_bounds__(256) void apply_rgba_fb_kernel(const uint32_t *__restrict__ lmap, const uint8_t *__restrict__ tints, const BkFbPlates src,
                                                            const BkFbGeom g, uint8_t *__restrict__ dst, int dst_pitch, const uint8_t *__restrict__ lut)
{
    BK_FB_LUT_S(lut);
    const int x = (int)blockIdx.x * 128 + (int)(threadIdx.x & 31u) * 4, row = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);
    if (row >= g.rows || x >= g.W) return;
    uint32_t o[4], t[4];
    bk_fb_entries<4, RUBIX>(lmap, tints, g, row, x, o, t);
    if ((o[0] & o[1] & o[2] & o[3]) == BK_NULL_OFFSET) return;
    const uint32_t *spare = lmap + (size_t)row * g.W + x;      // what an unmapped pixel loads instead of a texel
    const uint32_t *a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = o[k] != BK_NULL_OFFSET ? bk_fb_texel(src, g, o[k]) : spare;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *a[k];
    if (RUBIX) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = bk_fb_tint(v[k], t[k], lut_s);
    }
    uint8_t *out = dst + (size_t)row * dst_pitch + (size_t)x * 4;
    const bool all = o[0] != BK_NULL_OFFSET && o[1] != BK_NULL_OFFSET && o[2] != BK_NULL_OFFSET && o[3] != BK_NULL_OFFSET;      // (entries past W are NULL)
    BK_FB_STORE4(out, v, all, o[0] != BK_NULL_OFFSET, o[1] != BK_NULL_OFFSET, o[2] != BK_NULL_OFFSET, o[3] != BK_NULL_OFFSET);
}

// dst = pixel (0, 0) of the owned rows' part of the HALF-SIZE frame; grid = (ceil(Wo / 128), ceil(rows_o / 8)), Wo = (W + 1) / 2,
// rows_o = (rows + 1) / 2 (the owned rows begin on an even row: sample row 2 Y of the lensmap's owned part is the top of output row Y)
template <bool RUBIX>
__global__ __launch_bounds__(256) void apply_rgba_fb_ss2_kernel(const uint32_t *__restrict__ lmap, const uint8_t *__restrict__ tints, const BkFbPlates src,
                                                                const BkFbGeom g, uint8_t *__restrict__ dst, int dst_pitch, const uint8_t *__restrict__ lut)
{
    BK_FB_LUT_S(lut);
    const int xo = (int)blockIdx.x * 128 + (int)(threadIdx.x & 31u) * 4, yo = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);
    const int x = 2 * xo, row = 2 * yo;
    if (row >= g.rows || x >= g.W) return;
    uint32_t o[16], t[16];
    bk_fb_entries<8, RUBIX>(lmap, tints, g, row, x, o, t);
    if (row + 1 < g.rows) bk_fb_entries<8, RUBIX>(lmap, tints, g, row + 1, x, o + 8, t + 8);
    else {
#pragma unroll
        for (int k = 8; k < 16; ++k) { o[k] = BK_NULL_OFFSET; t[k] = 255u; }
    }
    uint32_t any = o[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) any &= o[k];
    if (any == BK_NULL_OFFSET) return;
    const uint32_t *spare = lmap + (size_t)row * g.W + x;
    const uint32_t *a[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = o[k] != BK_NULL_OFFSET ? bk_fb_texel(src, g, o[k]) : spare;
    uint32_t v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = *a[k];
    uint32_t px[4], n[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t lo = 0, hi = 0;      // bytes 0 / 2 and bytes 1 / 3 of the quad's samples, summed in 16-bit fields
        n[j] = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = (s >> 1) * 8 + 2 * j + (s & 1);
            if (o[k] != BK_NULL_OFFSET) {
                const uint32_t w = RUBIX ? bk_fb_tint(v[k], t[k], lut_s) : v[k];
                lo += w & 0x00FF00FFu;
                hi += (w >> 8) & 0x00FF00FFu;
                ++n[j];
            }
        }
        if (n[j] == 4u) {
            lo = ((lo + 0x00020002u) >> 2) & 0x00FF00FFu;
            hi = ((hi + 0x00020002u) >> 2) & 0x00FF00FFu;
        } else if (n[j]) {
            lo = bk_ss2_avg(lo & 0xFFFFu, n[j]) | (bk_ss2_avg(lo >> 16, n[j]) << 16);
            hi = bk_ss2_avg(hi & 0xFFFFu, n[j]) | (bk_ss2_avg(hi >> 16, n[j]) << 16);
        }
        px[j] = lo | (hi << 8);
    }
    uint8_t *out = dst + (size_t)yo * dst_pitch + (size_t)xo * 4;
    BK_FB_STORE4(out, px, n[0] && n[1] && n[2] && n[3], n[0], n[1], n[2], n[3]);      // (a quad past W has no sample)
}

// ---- BILINEAR (bk_apply_rgba_fb_bilinear_device) ----------------------------------------------------------------------------------
// The reference keeps trunc(u * ps) of a ray's position on its plate (fisheye.c:1988, after :2055-2062) and render_lensmap reads that one
// texel; the build can keep the eight fraction bits beside it (BkBuildParams::subtexel: qx | qy << 8), and this kernel blends the four
// texels around the position.  Texel centres sit at px + 1/2, so with sx = qx + 128 the left texel of the pair is px - 1 + (sx >> 8) and
// the right one's weight fx = sx & 255 (of 256); rows alike.  Both are clamped to the entry's OWN plate: no filtering across a cube seam.
// Integer and exact, per byte: h0 = a00 * (256 - fx) + a01 * fx, h1 = a10 * (256 - fx) + a11 * fx, out = (h0 * (256 - fy) + h1 * fy +
// 32768) >> 16.  Sub 0x8080 is fx = fy = 0 on the named texel itself: the nearest kernel's frame, byte for byte.
// Layout: apply_rgba_fb_kernel's - 128 x 8 pixels a workgroup, four consecutive pixels a lane, entries one 16-byte load, subs one
// 8-byte load (W % 4 == 0), ONE decode per pixel (bk_fb_locate), the three neighbours the same base with clamped coordinates; all
// sixteen addresses are formed before the first texel is used, an unmapped pixel's four are the lane's own lensmap entry.  The first
// stage runs on even and odd bytes as two 16-bit fields a dword (a field's sum is at most 255 * 256: no carry), two 24-bit multiplies
// each; the second per byte as (h0 << 8) + fy * (h1 - h0) - the same number - one signed 24-bit multiply.  Tinted: every one of the
// four texels goes through bk_fb_tint first, as ss2 tints per sample before its average.
// As built (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch): plain / tinted 49 / 66 VGPRs = 8 / 7 waves per SIMD.
// SEAMS (bk_apply_rgba_fb_bilinear_seams_device): the same common path, then one wave-uniform branch into the seam pass (below);
// as built 68 / 78 VGPRs = 7 / 6 waves per SIMD, no scratch - a wave less than the kernel without it, and the measured price: at 4K
// S / L = 1.12 / 1.03 / 1.08 plain and 1.14 / 1.14 / 1.14 tinted (panini / hammer / quincuncial), the target S <= L + both spreads
// MISSED everywhere (profiles/rgba_fb_bilinear_seams_apply.txt).  Suspected, not shown by a counter pass: the occupancy, since under
// 0.1 % of the pixels take the pass.  What was tried: the pass before the common loads (80 / 84), after them with the decode kept (84 / 90).
// Measured: tools/bench_rgba.py --fb --bilinear [--seams] [--tint], profiles/rgba_fb_bilinear_apply.txt.

// The geometry of one bilinear pixel, stated once for the common path and the seams pass: from its entry `off` and its sub `q` (and the
// kernel's src, g, ps_m1, spare) the weights fx, fy; as locals of the block it stands in `mapped`, the plate's number `plate`, the
// pair's right column xr = px + (sx >> 8) and lower row yr (the pairs are xr - 1, xr and yr - 1, yr, possibly a step outside the
// plate); and into a[0..3] the four addresses, row ya | yb, column xa | xb, clamped to the entry's own plate - `spare` all four for an
// unmapped pixel.  (A macro for BK_FB_PICK's reason.)
#define BK_FB_BILINEAR_AT(off, q, fx, fy, a)                                                                                       \
    const bool mapped = (off) != BK_NULL_OFFSET;                                                                                   \
    const uint8_t *base;                                                                                                           \
    uint32_t pitch, px, py;                                                                                                        \
    const uint32_t plate = bk_fb_locate(src, g, (off), base, pitch, px, py);                                                       \
    const uint32_t sx = ((q) & 255u) + 128u, sy = ((q) >> 8) + 128u;                                                               \
    (fx) = sx & 255u; (fy) = sy & 255u;                                                                                            \
    /* the pair px - 1 + (sx >> 8), + 1, clamped to the plate: the left one can only fall below 0, the right one only pass ps - 1 */ \
    const uint32_t xr = px + (sx >> 8), yr = py + (sy >> 8);                                                                       \
    const uint32_t xa = xr ? xr - 1u : 0u, ya = yr ? yr - 1u : 0u;                                                                 \
    const uint32_t xb = xr < ps_m1 ? xr : ps_m1, yb = yr < ps_m1 ? yr : ps_m1;                                                     \
    const uint8_t *ra = base + (size_t)ya * pitch, *rb = base + (size_t)yb * pitch;                                                \
    (a)[0] = mapped ? reinterpret_cast<const uint32_t *>(ra + (size_t)xa * 4u) : spare;                                            \
    (a)[1] = mapped ? reinterpret_cast<const uint32_t *>(ra + (size_t)xb * 4u) : spare;                                            \
    (a)[2] = mapped ? reinterpret_cast<const uint32_t *>(rb + (size_t)xa * 4u) : spare;                                            \
    (a)[3] = mapped ? reinterpret_cast<const uint32_t *>(rb + (size_t)xb * 4u) : spare

// SEAMS: the four positions of pixel k (a[0..3]: row ya | yb, column xa | xb, already formed clamped to the pixel's own plate) that lie
// OUTSIDE that plate, through the seam table: seam = uint2 [6][4][n1] {plate * pb or 0xFFFFFFFF, py << 16 | px}, n1 = ps + 2, edge 0 = row -1,
// 1 = row ps, 2 = column -1, 3 = column ps, index = the coordinate along the edge + 1; a position outside in both axes is the row
// edge's corner entry.  A NULL entry, or one into a plate passed as NULL, leaves the clamped address.  xr = px + (sx >> 8), yr alike: the
// pair of columns is xr - 1, xr.  Every lane of the wave issues the four table loads (a lane with nothing outside reads entry 0 and
// drops it): no load hangs on a divergent branch.  The target's plate arrives as plate * pb, an offset for BK_FB_PICK.
__device__ __forceinline__ void bk_fb_seam_resolve(const BkFbPlates &s, const BkFbGeom &g, const uint2 *__restrict__ seam, uint32_t n1, bool mapped, uint32_t plate,
                                                   uint32_t xr, uint32_t yr, uint32_t ps_m1, const uint32_t *a[4])
{
    // (one position at a time, each behind a compiler barrier: the path is rare, and nothing is gained by four entries in flight)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t jx = (uint32_t)j & 1u, jy = (uint32_t)j >> 1;
        const bool ox = jx ? xr > ps_m1 : xr == 0u, oy = jy ? yr > ps_m1 : yr == 0u;
        const bool out = mapped && (ox || oy);
        const uint32_t edge = oy ? jy : 2u + jx, along = oy ? xr + jx : yr + jy;
        const uint2 e = seam[out ? (plate * 4u + edge) * n1 + (along < n1 ? along : n1 - 1u) : 0u];
        const uint8_t *base;
        uint32_t pitch, target;
        BK_FB_PICK(e.x, target, base, pitch);
        (void)target;
        const uint32_t *t = reinterpret_cast<const uint32_t *>(base + (size_t)(e.y >> 16) * pitch + (size_t)(e.y & 0xFFFFu) * 4u);
        a[j] = out && e.x != BK_NULL_OFFSET && base ? t : a[j];
        asm volatile("" ::: "memory");
    }
}

// the blend of one pixel: a00 a01 (upper row), a10 a11 (lower row), weights fx, fy in 0..255 of 256
__device__ __forceinline__ uint32_t bk_fb_blend(uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11, uint32_t fx, uint32_t fy)
{
    const uint32_t m = 0x00FF00FFu, gx = 256u - fx;
    // bytes 0 / 2 and bytes 1 / 3 as 16-bit fields: every operand below 2^24, every field's sum at most 65280
    const uint32_t h0e = __umul24(a00 & m, gx) + __umul24(a01 & m, fx), h0o = __umul24((a00 >> 8) & m, gx) + __umul24((a01 >> 8) & m, fx);
    const uint32_t h1e = __umul24(a10 & m, gx) + __umul24(a11 & m, fx), h1o = __umul24((a10 >> 8) & m, gx) + __umul24((a11 >> 8) & m, fx);
    // h0 * (256 - fy) + h1 * fy = (h0 << 8) + fy * (h1 - h0), |h1 - h0| <= 65280: a signed 24-bit product; the sum is below 2^24 + 2^15
#define BK_FB_STAGE2(h0, h1) ((uint32_t)((int)((h0) << 8) + __mul24((int)(h1) - (int)(h0), (int)fy) + 32768) >> 16)
    const uint32_t b0 = BK_FB_STAGE2(h0e & 0xFFFFu, h1e & 0xFFFFu), b2 = BK_FB_STAGE2(h0e >> 16, h1e >> 16);
    const uint32_t b1 = BK_FB_STAGE2(h0o & 0xFFFFu, h1o & 0xFFFFu), b3 = BK_FB_STAGE2(h0o >> 16, h1o >> 16);
#undef BK_FB_STAGE2
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// sub = the sub-texel plane, [rows][W] as lmap; ps_m1 = platesize - 1; otherwise apply_rgba_fb_kernel's arguments and grid;
// SEAMS: seam = the decoded seam table (bk_fb_seam_resolve; unused and NULL otherwise)
template <bool RUBIX, bool SEAMS>
__global__ __launch_bounds__(256) void apply_rgba_fb_bilinear_kernel(const uint32_t *__restrict__ lmap, const uint8_t *__restrict__ tints,
                                                                     const uint16_t *__restrict__ sub, const BkFbPlates src, const BkFbGeom g, uint32_t ps_m1,
                                                                     uint8_t *__restrict__ dst, int dst_pitch, const uint8_t *__restrict__ lut,
                                                                     const uint2 *__restrict__ seam)
{
    BK_FB_LUT_S(lut);
    const int x = (int)blockIdx.x * 128 + (int)(threadIdx.x & 31u) * 4, row = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);
    if (row >= g.rows || x >= g.W) return;
    uint32_t o[4], t[4], q[4];
    bk_fb_entries<4, RUBIX>(lmap, tints, g, row, x, o, t);
    const size_t at = (size_t)row * g.W + x;
    if (g.lmap4) {                                   // (x + 3 < W; at % 4 == 0: eight aligned bytes)
        const uint2 s2 = *reinterpret_cast<const uint2 *>(sub + at);
        q[0] = s2.x & 0xFFFFu; q[1] = s2.x >> 16; q[2] = s2.y & 0xFFFFu; q[3] = s2.y >> 16;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = x + k < g.W ? (uint32_t)sub[at + k] : 0x8080u;
    }
    if ((o[0] & o[1] & o[2] & o[3]) == BK_NULL_OFFSET) return;
    const uint32_t *spare = lmap + at;               // what an unmapped pixel loads instead of its texels
    const uint32_t *a[16];
    uint32_t fx[4], fy[4];
    bool rim = false;                                // SEAMS: one of the lane's sixteen positions lies outside its pixel's plate
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        BK_FB_BILINEAR_AT(o[k], q[k], fx[k], fy[k], a + 4 * k);
        (void)plate;
        if (SEAMS) rim |= mapped && (xr == 0u || yr == 0u || xr > ps_m1 || yr > ps_m1);
    }
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = *a[k];
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (RUBIX) {
#pragma unroll
            for (int j = 0; j < 4; ++j) w[4 * k + j] = bk_fb_tint(w[4 * k + j], t[k], lut_s);
        }
        v[k] = bk_fb_blend(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3], fx[k], fy[k]);
    }
    // SEAMS.  Everything up to here is the kernel without it: every pixel blended from its own plate, clamped.  The seam table's dependent
    // loads (entry -> plate base and pitch -> address) are taken only by a wave that has a lane on a rim - one uniform branch, under 1 %
    // of the waves of a 4K frame - and AFTER the common path, when its sixteen addresses and texels are dead: such a wave makes its pixels
    // again, one at a time, from the entry and the sub (BK_FB_BILINEAR_AT again, the addresses outside the plate replaced through the
    // table, four loads, tint, blend).  That was meant to keep the pass's registers below the common path's; as built it does not: the
    // kernel takes 68 / 78 VGPRs where the one without SEAMS takes 49 / 66, a wave per SIMD less (the head comment has what it costs).
    // A pixel with nothing outside its plate comes out as it was.
    if (SEAMS && __any(rim)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // (the entry and the sub as values the compiler has not seen: otherwise it keeps the common path's decode of all four pixels
            //  alive down to here instead of taking it again: 84 / 90 VGPRs)
            uint32_t ok = o[k], qk = q[k];
            asm volatile("" : "+v"(ok), "+v"(qk));
            uint32_t fxk, fyk;
            const uint32_t *b[4];
            BK_FB_BILINEAR_AT(ok, qk, fxk, fyk, b);
            bk_fb_seam_resolve(src, g, seam, ps_m1 + 3u, mapped, plate, xr, yr, ps_m1, b);
            uint32_t c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = *b[j];
            if (RUBIX) {
#pragma unroll
                for (int j = 0; j < 4; ++j) c[j] = bk_fb_tint(c[j], t[k], lut_s);
            }
            v[k] = bk_fb_blend(c[0], c[1], c[2], c[3], fxk, fyk);
            asm volatile("" ::: "memory");           // (one pixel at a time: four pixels' table entries and texels in flight are registers)
        }
    }
    uint8_t *out = dst + (size_t)row * dst_pitch + (size_t)x * 4;
    const bool all = o[0] != BK_NULL_OFFSET && o[1] != BK_NULL_OFFSET && o[2] != BK_NULL_OFFSET && o[3] != BK_NULL_OFFSET;      // (entries past W are NULL)
    BK_FB_STORE4(out, v, all, o[0] != BK_NULL_OFFSET, o[1] != BK_NULL_OFFSET, o[2] != BK_NULL_OFFSET, o[3] != BK_NULL_OFFSET);
}

// The one launch of this file.  dst = pixel (x0, y0 + row0) of the frame - FB_SS2: (x0, y0 + row0 / 2) of the half-size frame; plates /
// pitches: validated by the caller (a NULL plate is one no entry of the owned rows names); d_lut != nullptr: the tinted launch.  Both
// bilinear modes: the caller has made sure of the sub-texel plane; FB_BILINEAR_SEAMS: and has made ctx->d_seam current
int launch_apply_rgba_fb(bk_ctx *ctx, const void *const plates[BK_MAX_PLATES], const int pitches[BK_MAX_PLATES], uint8_t *dst, int dst_pitch,
                         const uint8_t *d_lut, FbMode mode)
{
    if (mode == FB_BILINEAR_SEAMS &&
        (!ctx->d_seam || !ctx->d_seam_current || ctx->seam_table.size() != (size_t)BK_MAX_PLATES * 4u * ((size_t)ctx->ps + 2u)))
        return ctx->fail(BK_E_STATE, "bk_apply_rgba_fb_bilinear_seams_device: the seam table on the device is not the current one");
    const int rows = ctx->rows();
    if (rows <= 0 || ctx->W <= 0) return BK_OK;
    BkFbPlates src;
    for (int p = 0; p < BK_MAX_PLATES; ++p) {
        src.p[p] = (const uint8_t *)plates[p];
        src.pitch[p] = plates[p] ? (uint32_t)pitches[p] : 0u;
    }
    BkFbGeom g;
    g.pb = (uint32_t)ctx->gp * (uint32_t)ctx->ph;
    g.tpr = (uint32_t)ctx->gp >> 4;
    g.tpr_m = bk_fb_recip(g.tpr);
    g.W = ctx->W;
    g.rows = rows;
    g.lmap4 = (ctx->W & 3) == 0;
    const uint32_t ps_m1 = (uint32_t)ctx->ps - 1u;
    const int w = mode == FB_SS2 ? (ctx->W + 1) / 2 : ctx->W, h = mode == FB_SS2 ? (rows + 1) / 2 : rows;
    const dim3 grid((unsigned)((w + 127) / 128), (unsigned)((h + 7) / 8));
    const uint2 *seam = mode == FB_BILINEAR_SEAMS ? ctx->d_seam : nullptr;
    // the mode's kernel, tinted or plain.  (The cases stand in the order the eight kernels have always been instantiated in: with the
    // bilinear ones instantiated in another order the compiler allocates the seams kernels' registers differently.)
#define BK_FB_LAUNCH(tinted, plain, ...)                                                                                           \
    if (d_lut) hipLaunchKernelGGL(tinted, grid, dim3(256), 0, ctx->stream, ctx->d_offsets, ctx->d_tints, __VA_ARGS__);             \
    else hipLaunchKernelGGL(plain, grid, dim3(256), 0, ctx->stream, ctx->d_offsets, ctx->d_tints, __VA_ARGS__)
    switch (mode) {
    case FB_SS2:
        BK_FB_LAUNCH(apply_rgba_fb_ss2_kernel<true>, apply_rgba_fb_ss2_kernel<false>, src, g, dst, dst_pitch, d_lut);
        break;
    case FB_NEAREST:
        BK_FB_LAUNCH(apply_rgba_fb_kernel<true>, apply_rgba_fb_kernel<false>, src, g, dst, dst_pitch, d_lut);
        break;
    case FB_BILINEAR_SEAMS:
        BK_FB_LAUNCH((apply_rgba_fb_bilinear_kernel<true, true>), (apply_rgba_fb_bilinear_kernel<false, true>), ctx->d_subtexel, src, g, ps_m1, dst, dst_pitch,
                     d_lut, seam);
        break;
    case FB_BILINEAR:
        BK_FB_LAUNCH((apply_rgba_fb_bilinear_kernel<true, false>), (apply_rgba_fb_bilinear_kernel<false, false>), ctx->d_subtexel, src, g, ps_m1, dst, dst_pitch,
                     d_lut, seam);
        break;
    }
#undef BK_FB_LAUNCH
    BK_HIP(ctx, hipGetLastError());
    return BK_OK;
}
