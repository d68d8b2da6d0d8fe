// bk_apply_rgba_mip.inc -- part of bk_apply_coop.hip: the TRILINEAR truecolour apply from six row-major frame buffers
// (bk_apply_rgba_fb_trilinear_device) for gfx950 - the mip pyramid of the plates, the level-of-detail plane beside the lensmap, and the
// apply that blends two levels of the pyramid.  Everything is integer arithmetic; tests/trilinear_model.py is the numpy statement.
//
// THE PYRAMID (ctx->d_mip).  Level 0 is the caller's plate, s_0 = ps; s_{k+1} = (s_k + 1) / 2 down to 1 (bk::mip_layout, bk_api.cpp).
// Texel (x, y) of level k + 1, per byte: (a + b + c + d + 2) >> 2 over level k's (2x, 2y), (2x + 1, 2y), (2x, 2y + 1), (2x + 1, 2y + 1),
// coordinates clamped to s_k - 1; every level is made from the ROUNDED level below.  d_mip = uint4 [BK_MIP_MAX_LEVELS] {byte offset of
// level k inside a plate's part, its row pitch, s_k - 1, s_k} (level 0: 0, 0, ps - 1, ps), then six parts of plate_stride bytes; pitches
// are multiples of 16, level offsets and plate_stride of 128.
// Two launches a frame, not one per level:
//   mip_head_kernel: levels 1-3 from level 0.  A workgroup of 256 takes 128 x 16 texels of level 0: a thread two rows of four texels (two
//     16-byte loads where the plate's base and pitch allow and the four lie inside, eight clamped dword loads otherwise), its two level-1
//     texels into LDS and - 8 bytes a lane, a wave two whole 256-byte rows - into the pyramid; 128 threads then make the 32 x 4 level-2
//     texels out of the LDS copy, 32 threads the 16 x 2 of level 3.  The LDS copies are read at coordinates clamped to s_k - 1, as the rule
//     says: a tile's entries past the level's size are not that level's texels.  blockIdx.z = the plate; a NULL plate's workgroups leave.
//     Whole 128-byte lines per store instruction hold for LEVEL 1 only (level offsets and pitches allow it for every source class): levels
//     2 and 3 leave as one dword a lane, 128 and 64 bytes a row, two rows a wave - a twenty-first of the pyramid's bytes.
//   mip_tail_kernel: levels 4 .. L - 1, at most ps / 16 on a side, one workgroup of 1024 per plate, level after level with a barrier
//     between (its own writes, its own CU).  One dword load per source texel, one dword store and one integer division per texel made:
//     small and plain, and the suspected cause of the pyramid's missed rate (below); spreading level 4 over more workgroups is the follow-up.
// THE LEVEL OF DETAIL (ctx->d_lod, uint16 [rows][W] = level << 8 | fraction; lod_kernel): a pixel's position to 1/256 texel is
// U = px * 256 + qx, V = py * 256 + qy; its horizontal step goes to x + 1 if that is inside the frame, mapped and on the same plate, else
// to x - 1 under the same test, else there is none; the vertical step alike inside the OWNED rows; rho = max over both of max(|dU|, |dV|).
// rho <= 256: 0; else k = floor(log2 rho), (k - 8) * 256 + ((rho << 8) >> k) - 256.  Plus the bias, clamped to [0, (L - 1) * 256]; NULL: 0.
// THE APPLY (apply_rgba_fb_trilinear_kernel<RUBIX>): l = lod >> 8, fl = lod & 255, levels lo = l and hi = min(l + 1, L - 1).  At level k
// the position is (U >> k, V >> k), and (Uk >> 8, Uk & 255) are what (px, qx) are to the bilinear kernel: sx = q + 128, the pair of
// columns, the weight, clamped to [0, s_k - 1] of the pixel's own plate.  Per byte and level v = h0 * (256 - fy) + h1 * fy UNROUNDED
// (<= 255 * 65536); out = (v_lo * (256 - fl) + v_hi * fl + 2^23) >> 24, below 2^32 throughout.  fl = 0: (v_lo + 32768) >> 16 - a plane
// of zeros is the bilinear kernel's frame.  Tinted: each of the eight texels through bk_fb_tint before any blend.
// Layout: the family's - 128 x 8 pixels a workgroup, four consecutive pixels a lane, all 32 addresses formed before the first texel is
// used, an unmapped pixel's eight are the lane's own lensmap entry, BK_FB_STORE4.  Level 0 comes from the six by-value pointers
// (BK_FB_PICK), levels from 1 on from the pyramid; a level's offset, pitch and size come from a copy of d_mip's table in LDS (indexed by
// the level: the same index into a kernel argument is a copy of the argument in scratch, as bk_apply_rgba_fb.inc's head comment tells).
// As built (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any): the apply plain / tinted 98 / 122 VGPRs = 4 / 4 waves per
// SIMD (98 is allocated as 104); mip_head_kernel 28, mip_tail_kernel 23, lod_kernel 21 VGPRs = 8 waves.  bk_apply_rgba_fb.inc's eight kernels keep their figures.
// Measured (tools/bench_rgba.py --fb --trilinear [--tint], profiles/rgba_fb_trilinear_apply.txt; 4K, plates from HBM; L = the bilinear call,
// T0 / T = this call with mips 0 / 1, M = the pyramid by itself, bk_debug_mip_pyramid): hammer plain L 82.0, T0 89.4, T 157.1, M 73.4 us;
// quincuncial 83.0 / 95.1 / 157.5 / 73.3; winkel2 82.9 / 99.5 / 165.6 / 73.3; panini - every pixel's lower level is 0 there - 63.2 / 112.0 /
// 170.0 / 65.2; tinted hammer 79.0 / 100.6 / 169.4 / 74.1.  No ratio was fixed.  T0 / L = 1.09 - 1.20 on the minifying lenses: eight texels
// for little more than four, as expected; 1.77 on panini (suspected: 4 waves per SIMD for L's 8 / 7, sixteen more loads a lane).  M moves
// 149.3 MB at 2.03 TB/s (2.21 counted as T - T0) where plate_rgba_retile_footprint_kernel reaches 2.87 on hammer: MISSED (suspected: the
// tail's six workgroups working through levels 4 .. 12 alone on the chip, and the launch gap in front of them).  Neither suspicion has been
// measured.  DESIGN.md 3.1 has the table.

struct BkMipHead {
    uint32_t s0, L;                               // ps, levels (level 0 included)
    uint32_t off1, pitch1, s1, off2, pitch2, s2, off3, pitch3, s3;      // of levels 1-3 (named, not indexed); unused beyond L - 1
    size_t plate_stride;
};

// the rounded mean of four texels, per byte: even and odd bytes as 16-bit fields (a field's sum is at most 4 * 255 + 2)
__device__ __forceinline__ uint32_t bk_mip_avg4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t m = 0x00FF00FFu;
    const uint32_t e = (((a & m) + (b & m) + (c & m) + (d & m) + 0x00020002u) >> 2) & m;
    const uint32_t o = ((((a >> 8) & m) + ((b >> 8) & m) + ((c >> 8) & m) + ((d >> 8) & m) + 0x00020002u) >> 2) & m;
    return e | (o << 8);
}

// mip = the first plate's part of the pyramid; grid = (ceil(ps / 128), ceil(ps / 16), 6)
__global__ __launch_bounds__(256) void mip_head_kernel(const BkFbPlates src, const BkMipHead h, uint8_t *__restrict__ mip)
{
    __shared__ uint32_t l1[8][64], l2[4][32];
    const uint32_t plate = blockIdx.z;            // (uniform: the argument is read where it lies, no copy)
    const uint8_t *base = src.p[plate];
    if (!base || h.L < 2u) return;
    const uint32_t pitch = src.pitch[plate];
    uint8_t *out = mip + (size_t)plate * h.plate_stride;
    const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
    const uint32_t X0 = blockIdx.x * 128u, Y0 = blockIdx.y * 16u, sm = h.s0 - 1u;      // (X0, Y0 < ps: the tile's first texel exists on every level)
    const uint32_t x = X0 + 4u * tx, y = Y0 + 2u * ty;
    const uint8_t *ra = base + (size_t)(y < sm ? y : sm) * pitch, *rb = base + (size_t)(y + 1u < sm ? y + 1u : sm) * pitch;
    uint32_t a[4], b[4];
    if (x + 3u <= sm && ((reinterpret_cast<uintptr_t>(ra + (size_t)x * 4u) | reinterpret_cast<uintptr_t>(rb + (size_t)x * 4u)) & 15u) == 0) {
        const uint4 qa = *reinterpret_cast<const uint4 *>(ra + (size_t)x * 4u), qb = *reinterpret_cast<const uint4 *>(rb + (size_t)x * 4u);
        a[0] = qa.x; a[1] = qa.y; a[2] = qa.z; a[3] = qa.w;
        b[0] = qb.x; b[1] = qb.y; b[2] = qb.z; b[3] = qb.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t xc = x + j < sm ? x + j : sm;
            a[j] = reinterpret_cast<const uint32_t *>(ra)[xc];
            b[j] = reinterpret_cast<const uint32_t *>(rb)[xc];
        }
    }
    const uint32_t v0 = bk_mip_avg4(a[0], a[1], b[0], b[1]), v1 = bk_mip_avg4(a[2], a[3], b[2], b[3]);
    l1[ty][2u * tx] = v0;
    l1[ty][2u * tx + 1u] = v1;
    const uint32_t x1 = (X0 >> 1) + 2u * tx, y1 = (Y0 >> 1) + ty;
    if (y1 < h.s1) {
        uint8_t *row = out + h.off1 + (size_t)y1 * h.pitch1 + (size_t)x1 * 4u;      // (x1 even, offset and pitch multiples of 16: 8-byte aligned)
        if (x1 + 1u < h.s1) *reinterpret_cast<uint2 *>(row) = make_uint2(v0, v1);
        else if (x1 < h.s1) *reinterpret_cast<uint32_t *>(row) = v0;
    }
    if (h.L < 3u) return;                         // (uniform)
    __syncthreads();
    if (threadIdx.x < 128u) {
        const uint32_t xl = threadIdx.x & 31u, yl = threadIdx.x >> 5, x2 = (X0 >> 2) + xl, y2 = (Y0 >> 2) + yl, s1m = h.s1 - 1u;
        // level 1's coordinates clamped to s1 - 1, then inside the tile: at least its origin (X0 / 2 <= s1 - 1), at most 2 * xl + 1
        const uint32_t xa = (2u * x2 < s1m ? 2u * x2 : s1m) - (X0 >> 1), xb = (2u * x2 + 1u < s1m ? 2u * x2 + 1u : s1m) - (X0 >> 1);
        const uint32_t ya = (2u * y2 < s1m ? 2u * y2 : s1m) - (Y0 >> 1), yb = (2u * y2 + 1u < s1m ? 2u * y2 + 1u : s1m) - (Y0 >> 1);
        const uint32_t v = bk_mip_avg4(l1[ya][xa], l1[ya][xb], l1[yb][xa], l1[yb][xb]);
        l2[yl][xl] = v;
        if (x2 < h.s2 && y2 < h.s2) *reinterpret_cast<uint32_t *>(out + h.off2 + (size_t)y2 * h.pitch2 + (size_t)x2 * 4u) = v;
    }
    if (h.L < 4u) return;
    __syncthreads();
    if (threadIdx.x < 32u) {
        const uint32_t xl = threadIdx.x & 15u, yl = threadIdx.x >> 4, x3 = (X0 >> 3) + xl, y3 = (Y0 >> 3) + yl, s2m = h.s2 - 1u;
        const uint32_t xa = (2u * x3 < s2m ? 2u * x3 : s2m) - (X0 >> 2), xb = (2u * x3 + 1u < s2m ? 2u * x3 + 1u : s2m) - (X0 >> 2);
        const uint32_t ya = (2u * y3 < s2m ? 2u * y3 : s2m) - (Y0 >> 2), yb = (2u * y3 + 1u < s2m ? 2u * y3 + 1u : s2m) - (Y0 >> 2);
        if (x3 < h.s3 && y3 < h.s3)
            *reinterpret_cast<uint32_t *>(out + h.off3 + (size_t)y3 * h.pitch3 + (size_t)x3 * 4u) = bk_mip_avg4(l2[ya][xa], l2[ya][xb], l2[yb][xa], l2[yb][xb]);
    }
}

// levels 4 .. L - 1 of plate blockIdx.x out of its level 3; tab = d_mip's table; skip: bit p = plate p was NULL; grid = 6
__global__ __launch_bounds__(1024) void mip_tail_kernel(uint8_t *__restrict__ mip, const uint4 *__restrict__ tab, uint32_t L, size_t plate_stride, uint32_t skip)
{
    if ((skip >> blockIdx.x) & 1u) return;
    uint8_t *part = mip + (size_t)blockIdx.x * plate_stride;
    for (uint32_t k = 4; k < L; ++k) {
        const uint4 s = tab[k - 1u], d = tab[k];
        const uint32_t n = d.w * d.w;             // (d.w <= ps / 16 < 2^11)
        for (uint32_t i = threadIdx.x; i < n; i += 1024u) {
            const uint32_t yy = i / d.w, xx = i - yy * d.w;
            const uint32_t xa = 2u * xx < s.z ? 2u * xx : s.z, xb = 2u * xx + 1u < s.z ? 2u * xx + 1u : s.z;
            const uint32_t ya = 2u * yy < s.z ? 2u * yy : s.z, yb = 2u * yy + 1u < s.z ? 2u * yy + 1u : s.z;
            const uint32_t *ra = reinterpret_cast<const uint32_t *>(part + s.x + (size_t)ya * s.y), *rb = reinterpret_cast<const uint32_t *>(part + s.x + (size_t)yb * s.y);
            reinterpret_cast<uint32_t *>(part + d.x + (size_t)yy * d.y)[xx] = bk_mip_avg4(ra[xa], ra[xb], rb[xa], rb[xb]);
        }
        __syncthreads();                          // (level k is whole, and visible to this workgroup, before level k + 1 reads it)
    }
}

// ---- the level-of-detail plane ---------------------------------------------------------------------------------------------------------
// entry `at` of the owned rows' lensmap: mapped?, and then its plate and its position in 1/256 texel
__device__ __forceinline__ bool bk_lod_pos(const uint32_t *__restrict__ lmap, const uint16_t *__restrict__ sub, const BkFbGeom &g, size_t at, uint32_t &plate, int &U, int &V)
{
    const uint32_t off = lmap[at];
    if (off == BK_NULL_OFFSET) return false;
    plate = BK_FB_PLATE(off, g.pb);
    uint32_t px, py;
    BK_FB_TEXEL(off - plate * g.pb, g.tpr, g.tpr_m, __umulhi, px, py);
    const uint32_t q = sub[at];
    U = (int)(px * 256u + (q & 255u));
    V = (int)(py * 256u + (q >> 8));
    return true;
}

// the step to the neighbour at `fwd` (if has_fwd, mapped and on `plate`), else at `bwd` under the same test, else 0
__device__ __forceinline__ int bk_lod_step(const uint32_t *__restrict__ lmap, const uint16_t *__restrict__ sub, const BkFbGeom &g, size_t fwd, bool has_fwd, size_t bwd,
                                           bool has_bwd, uint32_t plate, int U, int V)
{
    uint32_t p2;
    int U2, V2;
    if (has_fwd && bk_lod_pos(lmap, sub, g, fwd, p2, U2, V2) && p2 == plate) return max(abs(U2 - U), abs(V2 - V));
    if (has_bwd && bk_lod_pos(lmap, sub, g, bwd, p2, U2, V2) && p2 == plate) return max(abs(U2 - U), abs(V2 - V));
    return 0;
}

// bias: already clamped to +-2^20 (the clamp below swallows the rest); top = (L - 1) * 256; grid = ceil(rows * W / 256)
__global__ __launch_bounds__(256) void lod_kernel(const uint32_t *__restrict__ lmap, const uint16_t *__restrict__ sub, const BkFbGeom g, int bias, int top,
                                                  uint16_t *__restrict__ lod)
{
    const size_t at = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= (size_t)g.rows * g.W) return;
    const int row = (int)(at / (size_t)g.W), x = (int)(at - (size_t)row * g.W);
    uint32_t plate;
    int U, V;
    if (!bk_lod_pos(lmap, sub, g, at, plate, U, V)) { lod[at] = 0; return; }
    const int dh = bk_lod_step(lmap, sub, g, at + 1, x + 1 < g.W, at - 1, x > 0, plate, U, V);
    const int dv = bk_lod_step(lmap, sub, g, at + g.W, row + 1 < g.rows, at - g.W, row > 0, plate, U, V);
    const uint32_t rho = (uint32_t)max(dh, dv);   // (below 2^23: a plate is at most 26752 texels wide)
    int v = 0;
    if (rho > 256u) {
        const int k = 31 - __clz((int)rho);
        v = (k - 8) * 256 + (int)((rho << 8) >> k) - 256;
    }
    v += bias;
    lod[at] = (uint16_t)(v < 0 ? 0 : v > top ? top : v);
}

// ---- the apply ------------------------------------------------------------------------------------------------------------------------
// One pixel at one level: from its plate's level-0 base and pitch (base0, pitch0), its position (U, V) and the level's table entry the
// weights (fx | fy << 8) and the four addresses a[0..3] (row ya | yb, column xa | xb), clamped to the level; `spare` for an unmapped pixel
__device__ __forceinline__ uint32_t bk_mip_at(const uint4 *lv_s, uint32_t k, const uint8_t *base0, uint32_t pitch0, const uint8_t *part, uint32_t U, uint32_t V,
                                              bool mapped, const uint32_t *spare, const uint32_t *a[4])
{
    const uint4 e = lv_s[k];
    const uint8_t *base = k ? part + e.x : base0;
    const uint32_t pitch = k ? e.y : pitch0, sm1 = e.z;
    const uint32_t Uk = U >> k, Vk = V >> k;
    const uint32_t sx = (Uk & 255u) + 128u, sy = (Vk & 255u) + 128u;
    const uint32_t xr = (Uk >> 8) + (sx >> 8), yr = (Vk >> 8) + (sy >> 8);
    const uint32_t xa = xr ? xr - 1u : 0u, ya = yr ? yr - 1u : 0u;
    const uint32_t xb = xr < sm1 ? xr : sm1, yb = yr < sm1 ? yr : sm1;
    const uint8_t *ra = base + (size_t)ya * pitch, *rb = base + (size_t)yb * pitch;
    a[0] = mapped ? reinterpret_cast<const uint32_t *>(ra + (size_t)xa * 4u) : spare;
    a[1] = mapped ? reinterpret_cast<const uint32_t *>(ra + (size_t)xb * 4u) : spare;
    a[2] = mapped ? reinterpret_cast<const uint32_t *>(rb + (size_t)xa * 4u) : spare;
    a[3] = mapped ? reinterpret_cast<const uint32_t *>(rb + (size_t)xb * 4u) : spare;
    return (sx & 255u) | ((sy & 255u) << 8);
}

// one level's UNROUNDED blend, per byte: v[c] = h0 * (256 - fy) + h1 * fy; the first stage as bk_fb_blend's, on two 16-bit fields a dword
__device__ __forceinline__ void bk_mip_bilinear(uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11, uint32_t fx, uint32_t fy, uint32_t v[4])
{
    const uint32_t m = 0x00FF00FFu, gx = 256u - fx;
    const uint32_t h0e = __umul24(a00 & m, gx) + __umul24(a01 & m, fx), h0o = __umul24((a00 >> 8) & m, gx) + __umul24((a01 >> 8) & m, fx);
    const uint32_t h1e = __umul24(a10 & m, gx) + __umul24(a11 & m, fx), h1o = __umul24((a10 >> 8) & m, gx) + __umul24((a11 >> 8) & m, fx);
#define BK_MIP_STAGE2(h0, h1) ((uint32_t)((int)((h0) << 8) + __mul24((int)(h1) - (int)(h0), (int)fy)))
    v[0] = BK_MIP_STAGE2(h0e & 0xFFFFu, h1e & 0xFFFFu); v[2] = BK_MIP_STAGE2(h0e >> 16, h1e >> 16);
    v[1] = BK_MIP_STAGE2(h0o & 0xFFFFu, h1o & 0xFFFFu); v[3] = BK_MIP_STAGE2(h0o >> 16, h1o >> 16);
#undef BK_MIP_STAGE2
}

// sub, lod = the two planes beside lmap; part0 = the first plate's part of the pyramid, tab = its table, top = L - 1; otherwise
// apply_rgba_fb_kernel's arguments and grid
template <bool RUBIX>
__global__ __launch_bounds__(256) void apply_rgba_fb_trilinear_kernel(const uint32_t *__restrict__ lmap, const uint8_t *__restrict__ tints,
                                                                      const uint16_t *__restrict__ sub, const uint16_t *__restrict__ lod, const BkFbPlates src,
                                                                      const BkFbGeom g, const uint8_t *__restrict__ part0, size_t plate_stride,
                                                                      const uint4 *__restrict__ tab, uint32_t top, uint8_t *__restrict__ dst, int dst_pitch,
                                                                      const uint8_t *__restrict__ lut)
{
    __shared__ uint4 lv_s[BK_MIP_MAX_LEVELS];
    if (threadIdx.x < (uint32_t)BK_MIP_MAX_LEVELS) lv_s[threadIdx.x] = tab[threadIdx.x];
    BK_FB_LUT_S(lut);                                // (tinted: its barrier covers the table too)
    if (!RUBIX) __syncthreads();
    const int x = (int)blockIdx.x * 128 + (int)(threadIdx.x & 31u) * 4, row = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);
    if (row >= g.rows || x >= g.W) return;
    uint32_t o[4], t[4], q[4], d[4];
    bk_fb_entries<4, RUBIX>(lmap, tints, g, row, x, o, t);
    const size_t at = (size_t)row * g.W + x;
    if (g.lmap4) {                                   // (x + 3 < W; at % 4 == 0: eight aligned bytes of each plane)
        const uint2 s2 = *reinterpret_cast<const uint2 *>(sub + at), d2 = *reinterpret_cast<const uint2 *>(lod + at);
        q[0] = s2.x & 0xFFFFu; q[1] = s2.x >> 16; q[2] = s2.y & 0xFFFFu; q[3] = s2.y >> 16;
        d[0] = d2.x & 0xFFFFu; d[1] = d2.x >> 16; d[2] = d2.y & 0xFFFFu; d[3] = d2.y >> 16;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[k] = x + k < g.W ? (uint32_t)sub[at + k] : 0x8080u;
            d[k] = x + k < g.W ? (uint32_t)lod[at + k] : 0u;
        }
    }
    if ((o[0] & o[1] & o[2] & o[3]) == BK_NULL_OFFSET) return;
    const uint32_t *spare = lmap + at;               // what an unmapped pixel loads instead of its texels
    const uint32_t *a[32];
    uint32_t f[8];                                   // fx | fy << 8 of pixel k at its lower (2k) and upper (2k + 1) level
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool mapped = o[k] != BK_NULL_OFFSET;
        const uint8_t *base;
        uint32_t pitch, px, py;
        const uint32_t plate = bk_fb_locate(src, g, o[k], base, pitch, px, py);
        const uint32_t U = px * 256u + (q[k] & 255u), V = py * 256u + (q[k] >> 8);
        const uint32_t l = (d[k] >> 8) < top ? (d[k] >> 8) : top, hi = l < top ? l + 1u : top;      // (a plane's levels are at most top: the first clamp changes nothing)
        const uint8_t *part = part0 + (size_t)plate * plate_stride;
        f[2 * k] = bk_mip_at(lv_s, l, base, pitch, part, U, V, mapped, spare, a + 8 * k);
        f[2 * k + 1] = bk_mip_at(lv_s, hi, base, pitch, part, U, V, mapped, spare, a + 8 * k + 4);
    }
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) w[k] = *a[k];
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (RUBIX) {
#pragma unroll
            for (int j = 0; j < 8; ++j) w[8 * k + j] = bk_fb_tint(w[8 * k + j], t[k], lut_s);
        }
        uint32_t vl[4], vh[4];
        bk_mip_bilinear(w[8 * k], w[8 * k + 1], w[8 * k + 2], w[8 * k + 3], f[2 * k] & 255u, f[2 * k] >> 8, vl);
        bk_mip_bilinear(w[8 * k + 4], w[8 * k + 5], w[8 * k + 6], w[8 * k + 7], f[2 * k + 1] & 255u, f[2 * k + 1] >> 8, vh);
        const uint32_t fl = d[k] & 255u, gl = 256u - fl;
        // v < 2^24 and a weight <= 256: 24-bit products; the sum is at most 255 * 2^24 + 2^23
#define BK_MIP_OUT(c) ((__umul24(vl[c], gl) + __umul24(vh[c], fl) + 0x800000u) >> 24)
        v[k] = BK_MIP_OUT(0) | (BK_MIP_OUT(1) << 8) | (BK_MIP_OUT(2) << 16) | (BK_MIP_OUT(3) << 24);
#undef BK_MIP_OUT
    }
    uint8_t *out = dst + (size_t)row * dst_pitch + (size_t)x * 4;
    const bool all = o[0] != BK_NULL_OFFSET && o[1] != BK_NULL_OFFSET && o[2] != BK_NULL_OFFSET && o[3] != BK_NULL_OFFSET;      // (entries past W are NULL)
    BK_FB_STORE4(out, v, all, o[0] != BK_NULL_OFFSET, o[1] != BK_NULL_OFFSET, o[2] != BK_NULL_OFFSET, o[3] != BK_NULL_OFFSET);
}

// ---- the launches -----------------------------------------------------------------------------------------------------------------------
static BkFbGeom mip_geom(bk_ctx *ctx)
{
    BkFbGeom g;
    g.pb = (uint32_t)ctx->gp * (uint32_t)ctx->ph;
    g.tpr = (uint32_t)ctx->gp >> 4;
    g.tpr_m = bk_fb_recip(g.tpr);
    g.W = ctx->W;
    g.rows = ctx->rows();
    g.lmap4 = (ctx->W & 3) == 0;
    return g;
}

// levels 1 .. L - 1 of the plates given (a NULL plate's levels stay as they are) into ctx->d_mip, which the caller has allocated for ctx->ps
int launch_mip_pyramid(bk_ctx *ctx, const void *const plates[BK_MAX_PLATES], const int pitches[BK_MAX_PLATES])
{
    const int L = ctx->mip_levels;
    if (L < 2) return BK_OK;
    BkFbPlates src;
    uint32_t skip = 0;
    for (int p = 0; p < BK_MAX_PLATES; ++p) {
        src.p[p] = (const uint8_t *)plates[p];
        src.pitch[p] = plates[p] ? (uint32_t)pitches[p] : 0u;
        if (!plates[p]) skip |= 1u << p;
    }
    const uint32_t (*t)[4] = ctx->mip_table;
    BkMipHead h = {};
    h.s0 = (uint32_t)ctx->ps; h.L = (uint32_t)L;
    h.off1 = t[1][0]; h.pitch1 = t[1][1]; h.s1 = t[1][3];
    if (L > 2) { h.off2 = t[2][0]; h.pitch2 = t[2][1]; h.s2 = t[2][3]; }
    if (L > 3) { h.off3 = t[3][0]; h.pitch3 = t[3][1]; h.s3 = t[3][3]; }
    h.plate_stride = ctx->mip_plate_stride;
    uint8_t *part0 = ctx->d_mip + BK_MIP_TABLE_BYTES;
    const dim3 grid((unsigned)((ctx->ps + 127) / 128), (unsigned)((ctx->ps + 15) / 16), BK_MAX_PLATES);
    hipLaunchKernelGGL(mip_head_kernel, grid, dim3(256), 0, ctx->stream, src, h, part0);
    if (L > 4)
        hipLaunchKernelGGL(mip_tail_kernel, dim3(BK_MAX_PLATES), dim3(1024), 0, ctx->stream, part0, reinterpret_cast<const uint4 *>(ctx->d_mip), (uint32_t)L,
                           ctx->mip_plate_stride, skip);
    BK_HIP(ctx, hipGetLastError());
    return BK_OK;
}

// ctx->d_lod (allocated by the caller) from the lensmap, the sub-texel plane, the owned rows and the bias
int launch_lod(bk_ctx *ctx)
{
    const size_t px = (size_t)ctx->W * ctx->rows();
    if (!px) return BK_OK;
    const int bias = ctx->lod_bias < -(1 << 20) ? -(1 << 20) : ctx->lod_bias > (1 << 20) ? (1 << 20) : ctx->lod_bias;
    hipLaunchKernelGGL(lod_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_offsets, ctx->d_subtexel, mip_geom(ctx), bias,
                       (mip_level_count(ctx->ps) - 1) * 256, ctx->d_lod);
    BK_HIP(ctx, hipGetLastError());
    return BK_OK;
}

// the trilinear frame; the caller has made sure of the sub-texel plane, the level-of-detail plane and a pyramid for ctx->ps
int launch_apply_rgba_fb_trilinear(bk_ctx *ctx, const void *const plates[BK_MAX_PLATES], const int pitches[BK_MAX_PLATES], uint8_t *dst, int dst_pitch,
                                   const uint8_t *d_lut)
{
    const int rows = ctx->rows();
    if (rows <= 0 || ctx->W <= 0) return BK_OK;
    BkFbPlates src;
    for (int p = 0; p < BK_MAX_PLATES; ++p) {
        src.p[p] = (const uint8_t *)plates[p];
        src.pitch[p] = plates[p] ? (uint32_t)pitches[p] : 0u;
    }
    const dim3 grid((unsigned)((ctx->W + 127) / 128), (unsigned)((rows + 7) / 8));
    const uint8_t *part0 = ctx->d_mip + BK_MIP_TABLE_BYTES;
    const uint4 *tab = reinterpret_cast<const uint4 *>(ctx->d_mip);
    const uint32_t top = (uint32_t)ctx->mip_levels - 1u;
    if (d_lut)
        hipLaunchKernelGGL(apply_rgba_fb_trilinear_kernel<true>, grid, dim3(256), 0, ctx->stream, ctx->d_offsets, ctx->d_tints, ctx->d_subtexel, ctx->d_lod, src,
                           mip_geom(ctx), part0, ctx->mip_plate_stride, tab, top, dst, dst_pitch, d_lut);
    else
        hipLaunchKernelGGL(apply_rgba_fb_trilinear_kernel<false>, grid, dim3(256), 0, ctx->stream, ctx->d_offsets, ctx->d_tints, ctx->d_subtexel, ctx->d_lod, src,
                           mip_geom(ctx), part0, ctx->mip_plate_stride, tab, top, dst, dst_pitch, d_lut);
    BK_HIP(ctx, hipGetLastError());
    return BK_OK;
}
