// bk_apply_rgba.inc -- part of bk_apply_coop.hip: the TRUECOLOUR apply (bk_apply_rgba_device) for gfx950.
//
// A 32-bit globe is four byte planes in four consecutive slots of the globe ring: truecolour globe g = slots 4g .. 4g+3, slot 4g+c
// holds byte c of every texel in the 16x8-tile layout every other slot has (bk_texel_offset).  The lensmap, the block map - chunk
// lists, 16-bit LDS addresses, walk order, XCD bands - are therefore valid as they are for every plane, and a truecolour frame is
// four of the 8-bit gathers through the same block map: per plane the block's chunks are staged to LDS and gathered into four more
// accumulator bytes per pixel; after the fourth plane a lane's 4x4 bytes are transposed in registers (v_perm_b32) and leave as whole
// 32-bit pixels.  The bytes are opaque: RGBA, BGRA, any 4-byte texel warps the same way.
//
// Which pixels a lane takes: its ROW is the one coop_compile_kernel gives it, but of the row's 32 four-pixel groups (16 bytes of frame
// each) lane j of the row's 32/RG takes groups j, j + 32/RG, j + 2 * 32/RG ... instead of RG consecutive ones - it simply loads those
// groups' LDS addresses from the block map (rgba_load_idx) - so that store instruction r of a wave writes the contiguous 16-byte
// pieces r * 32/RG + j: whole 128-byte lines per instruction, as the 8-bit kernel's one store per lane does
// (16 truecolour frames of 4K panini take 224.6 us, the 64 8-bit frames of the same slots 224.4; hammer 426.0 / 431.5:
//  profiles/rgba_apply.txt, which also has what consecutive pixels per lane cost).
// One block per workgroup, the PLAIN block map as ensure_coopmap compiles and tunes it for a launch of 4 * nframes planes; a block
// visit serves max(1, fchunk / 4) truecolour frames, i.e. the block map is read once per about 8 planes as in the 8-bit batch
// launch.  No strided / persistent / LDS-DMA form.
// Blocks the staging does not serve - a chunk list larger than the launch's staging buffer, CF_SLOW blocks without a list - gather
// straight from the lensmap: four byte loads and one dword store per mapped pixel (rare on real lenses; no multi-pass form).
//
// RUBIX (bk_apply_rgba_tinted_device, apply_coop_rgba_tinted_kernel<RG>): a tint on truecolour texels is a byte -> byte table per (byte
// plane, plate) - uint8 lut[4][6][256] - so plane c of a tinted frame is the 8-bit rubix gather of slot 4g + c through LUT c: the launch
// runs over the TINTED block map (CoopMap::tinted: a chunk listed once per tint class, the class in the entry's low three bits), loads
// from entry & ~15 and sends the 16 staged bytes through row class - 1 of the plane's LUT on their way to LDS (bk_rgba_tint_chunk) - the
// four register-held chunks and the rounds above 1024 chunks alike.  Everything behind the barrier is the plain kernel's.
// Where the LUTs live: ONE plane's 1.5 KiB in LDS behind the staging buffer, not all four (6 KiB).  Plane c + 1's 384 dwords are
// requested in front of plane c + 1's chunk loads - right behind the barrier that ends plane c's staging pass, the last reader of LUT c -
// ride in two registers through plane c's gather and are committed in front of the barrier that ends it (the BK_COOP_PROLOGUE /
// BK_COOP_PAL_COMMIT pattern: request early, commit late; no barrier added per plane).  LDS per workgroup is then what the 8-bit tinted
// kernel takes, staging buffer + 1.5 KiB; four LUTs would take a CU's 160 KiB from 8 workgroups to 6 at 4K panini's 18 KiB and from
// 6 to 5 at hammer's 25 KiB.  As built (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any of them):
//     plain  RG 1 / 2 / 4: 52 / 60 / 77 VGPRs = 8 / 7 / 6 waves per SIMD (a workgroup is one wave per SIMD: as many workgroups per CU)
//     tinted RG 1 / 2 / 4: 73 / 79 / 94 VGPRs = 6 / 6 / 5 waves per SIMD; LDS 19.5 KiB at 4K panini (RG 4), 26.5 KiB at 4K hammer (RG 2):
//     8 and 6 workgroups per CU by LDS - in the tinted kernel the REGISTERS decide, 5 and 6.
// Blocks without staging look the pixel's tint up in the lensmap's tint plane and its four bytes in the LUTs in device memory.
// Measured (tools/bench_rgba.py --tint, profiles/rgba_tint_apply.txt; A' = the 64-frame 8-bit rubix launch over the same slots through
// the same palette, B = the plain truecolour launch): 4K hammer 440.9 us against A' 445.0 and B 400.3; 4K panini 270.4 us against
// A' 232.9 and B 212.4 - there the target (A' + its spread) is MISSED by 16 %: the same look-ups per chunk as A', hidden by 5 workgroups
// per CU where the 8-bit tinted kernel (64 VGPRs) has 8.  Asking for 6 waves (amdgpu_waves_per_eu) spills 60 bytes per lane at RG = 4.
//
// SUPERSAMPLING (bk_apply_rgba_ss2_device, the SS = true instantiations of both kernels): the lensmap is W x H, the frame written is
// (W + 1) / 2 x (H + 1) / 2, every pixel the rounded mean of the mapped samples of its 2x2 quad: (sum + n / 2) / n, n = 0 untouched -
// the full-size frame, 16 bytes per output pixel, is never stored.  The launch is the full-size one in everything but the kernel: block
// map (plain or tinted), tuning, frames per visit, grid, LDS.
// Lane pairing: a lane's row is wave * 2 RG + lane / LPR (LPR = 32 / RG), so rows 2k and 2k + 1 of a block are lanes l and l ^ LPR of one
// wave, and block heights and wave tiles are even: no quad crosses a wave.  Per plane a lane adds its row's two horizontal pairs of a
// four-pixel group into one dword - (v0 + v1) | (v2 + v3) << 16, two 9-bit fields - fetches the other row's dword from lane l ^ LPR and
// adds: both quad sums of the group, 10 bits each, for all four planes in 4 dwords per group.  The exchange is VALU, not the LDS pipe the
// byte gathers fill: DPP row_ror:8 fused into the add (RG = 4), v_permlane16_swap (RG = 2), v_permlane32_swap (RG = 1) - bk_ss2_partner.
// Which groups a lane takes, chosen for the stores: a row pair owns 32 groups = 64 output pixels = 256 bytes of one output row, and BOTH
// its lanes store - the even row's lanes groups 0-15, the odd row's groups 16-31, each lane NS = RG / 2 NEIGHBOURING groups of its half
// (RG = 4: groups 2 cx, 2 cx + 1 -> one 16-byte store; RG = 2: group cx -> one 8-byte store) - so every wave issues ONE wide store
// instruction per frame, all 64 lanes in it, whose runs are whole 128-byte lines (LPR lanes x 8 NS bytes); one row of the pair storing
// everything would be the same lines in twice the instructions at half the lanes.  RG = 1 has one group per lane: the even row's lanes
// store it, 32 lanes x 8 bytes = the pair's 256 bytes.  A lane therefore loads the addresses of its NS groups and of the NS its partner
// stores (rgba_load_idx), gathers its row's half of all RG, keeps the sums of its own NS only (4 NS dwords where the full-size kernel
// keeps 4 RG) and sends the other half over: RG / 2 exchanges per plane, no output pixel computed or written twice.
// Fully mapped, aligned tiles (the full-size kernel's condition, alignment of the half-size frame: 8 bytes for RG = 1 / 2, 16 for RG = 4):
// ((sum + 2) >> 2) on both fields at once, bytes gathered with v_perm_b32, non-temporal stores as above.  Elsewhere the mapped bits
// (address != 0xFFFF; out-of-screen samples carry it too) are summed and exchanged the same way, once per block, and every output pixel
// with n > 0 is one dword store, the division by n = 3 a multiply by 21846 >> 16 (bk_ss2_avg: exact for every sum that occurs).
// Blocks without staging: the even row's lane gathers both rows of its 4 RG consecutive pixels from the lensmap, quad by quad.
// As built (no scratch in any of them; the six full-size instantiations keep the figures above):
//     ss2 plain  RG 1 / 2 / 4: 55 / 62 / 79 VGPRs = 8 / 8 / 6 waves per SIMD
//     ss2 tinted RG 1 / 2 / 4: 79 / 79 / 95 VGPRs = 6 / 6 / 5 waves per SIMD
// Measured (tools/bench_rgba.py --ss2 [--tint], profiles/rgba_ss2_apply.txt; A = the full-size launch of 16 4K frames, B = this one over
// the same globes into 16 1920x1080 frames, B checked against the average of A first): plain panini 150.7 us against A 215.4, hammer 338.5
// against 422.5; tinted panini 222.5 against 271.5, hammer 432.5 against 437.2 - B <= A + A's spread on all four.

// the lane's 4 pixels of row group r as whole dwords: P[c] holds byte c of pixels 0..3 -> px[k] holds bytes 0..3 of pixel k
__device__ __forceinline__ void bk_rgba_transpose(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t px[4])
{
    // v_perm_b32 D = perm(S0, S1, sel): selector byte 0-3 picks that byte of S1, 4-7 byte (n - 4) of S0
    const uint32_t t0 = __builtin_amdgcn_perm(p1, p0, 0x05010400u);      // p0.b0 p1.b0 p0.b1 p1.b1
    const uint32_t t1 = __builtin_amdgcn_perm(p1, p0, 0x07030602u);      // p0.b2 p1.b2 p0.b3 p1.b3
    const uint32_t u0 = __builtin_amdgcn_perm(p3, p2, 0x05010400u);
    const uint32_t u1 = __builtin_amdgcn_perm(p3, p2, 0x07030602u);
    px[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);
    px[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
    px[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);
    px[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
}

// bk_tint_chunk for this kernel: the same sixteen look-ups, TGROUP words (4 * TGROUP byte reads and their addresses) in flight at a
// time - all sixteen at once put RG = 2 at 82 VGPRs (5 waves per SIMD); two words at a time: 79 (6)
template <int TGROUP>
__device__ __forceinline__ uint4 bk_rgba_tint_chunk(uint4 q, uint32_t e, const uint8_t *pal_s)
{
    const uint32_t cls = e & 7u;
    if (cls) {
        const uint8_t *row = pal_s + (cls - 1u) * 256u;
        uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = (uint32_t)row[w[i] & 0xFFu] | ((uint32_t)row[(w[i] >> 8) & 0xFFu] << 8) | ((uint32_t)row[(w[i] >> 16) & 0xFFu] << 16) |
                   ((uint32_t)row[w[i] >> 24] << 24);
            if (i % TGROUP == TGROUP - 1) asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
        }
        q = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return q;
}

// SS2: what lane l ^ LPR - the other row of this lane's row pair, same wave - holds in `x`.  All 64 lanes must be active.
// LPR = 8: rows of a pair are the halves of one 16-lane DPP row (row_ror:8); LPR = 16 / 32: gfx950's v_permlane16_swap / v_permlane32_swap
// of x with itself leave the even rows' (lower half's) x in every lane of r[0] and the odd rows' (upper half's) in r[1].  VALU all three:
// the LDS pipe, which the byte gathers keep busy, sees none of it (__shfl_xor would be a ds_bpermute_b32 each).
template <int LPR>
__device__ __forceinline__ uint32_t bk_ss2_partner(uint32_t x, bool odd)
{
#if defined(__gfx950__)
    if constexpr (LPR == 8) {
        (void)odd;
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128 /* row_ror:8 */, 0xF, 0xF, false);
    } else if constexpr (LPR == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
        return odd ? r[0] : r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
        return odd ? r[0] : r[1];
    }
#else
    (void)odd;
    return (uint32_t)__shfl_xor((int)x, LPR);
#endif
}

// SS2: (sum + n / 2) / n for n = 1 .. 4 and every sum up to 4 * 255 + 2, exactly: thirds by 21846 / 65536 (21846 * 3 = 65536 + 2: the
// quotient is exact while 2 * sum < 65536), the others are shifts (tests/test_apply_rgba_ss2_gpu.py runs every sum at every count)
__device__ __forceinline__ uint32_t bk_ss2_avg(uint32_t sum, uint32_t n)
{
    return ((sum + (n >> 1)) * (n == 3u ? 21846u : 65536u >> (n >> 1))) >> 16;
}

// truecolour frames of one staged block: four planes per frame through the one staging buffer, plane c + 1's chunks requested before
// plane c's gather (coop_frames does the same from frame to frame)
// RUBIX: `blist` / s0..s3 are entries of a TINTED block map (class in the low bits); pal_s = the 1.5 KiB behind the staging buffer that
// hold the LUT of the plane being staged, lut = the four planes' LUTs in device memory (see the head comment)
// SS: the 2x2 supersampling launch (head comment): dst, dst_pitch, frame_stride are the HALF-SIZE frames', row0 / xb / cx still the
// lane's place in the full-size table
template <int NQ, int RG, bool RUBIX, bool SS>
__device__ __forceinline__ void rgba_frames(const uint8_t *__restrict__ globe, size_t globe_stride, int tglobes, int globe0, int f_begin,
                                            int f_end, uint8_t *__restrict__ dst, int dst_pitch, size_t frame_stride, uint8_t *buf,
                                            const uint32_t *__restrict__ blist, uint32_t nchunks, uint32_t s0, uint32_t s1, uint32_t s2,
                                            uint32_t s3, bool k0, bool k1, bool k2, bool k3, const CoopIdx<RG> ix, bool fast_store,
                                            bool tile_empty, int row0, int xb, int cx, const uint8_t *__restrict__ lut, uint8_t *pal_s)
{
    // ix.iw[r] = the LDS addresses of the row's four-pixel group r * LPR + cx (rgba_load_idx); xb = the block's first pixel column
    constexpr int LPR = 32 / RG;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0, q2 = q0, q3 = q0;      // (scalars, not an array: they must stay in VGPRs)
#define BK_RGBA_PLANE(F, C) (globe + (size_t)(4 * ((globe0 + (F)) % tglobes) + (C)) * globe_stride)
#define BK_RGBA_LOADS(F, C)                                                                    \
    do {                                                                                       \
        const uint8_t *gl_ = BK_RGBA_PLANE(F, C);                                              \
        q0 = *reinterpret_cast<const uint4 *>(gl_ + BK_CHUNK_OFF(s0));                         \
        if (NQ > 1) q1 = *reinterpret_cast<const uint4 *>(gl_ + BK_CHUNK_OFF(s1));             \
        if (NQ > 2) q2 = *reinterpret_cast<const uint4 *>(gl_ + BK_CHUNK_OFF(s2));             \
        if (NQ > 3) q3 = *reinterpret_cast<const uint4 *>(gl_ + BK_CHUNK_OFF(s3));             \
    } while (0)
    // RUBIX: plane C's LUT - 384 dwords, one and a half per thread - is REQUESTED in front of the plane's chunk loads and COMMITTED to
    // pal_s behind the previous plane's gather, where every wave is past the barrier that ends the staging pass which read the LUT before it
    uint32_t pal_r0 = 0, pal_r1 = 0;
#define BK_RGBA_LUT_REQUEST(C)                                                                 \
    do {                                                                                       \
        if (RUBIX) {                                                                           \
            const uint32_t *l_ = reinterpret_cast<const uint32_t *>(lut + (C) * BK_PAL_BYTES); \
            pal_r0 = l_[threadIdx.x];                                                          \
            if (threadIdx.x < BK_PAL_BYTES / 4 - 256) pal_r1 = l_[256 + threadIdx.x];          \
        }                                                                                      \
    } while (0)
#define BK_RGBA_LUT_COMMIT()                                                                   \
    do {                                                                                       \
        if (RUBIX) {                                                                           \
            reinterpret_cast<uint32_t *>(pal_s)[threadIdx.x] = pal_r0;                         \
            if (threadIdx.x < BK_PAL_BYTES / 4 - 256) reinterpret_cast<uint32_t *>(pal_s)[256 + threadIdx.x] = pal_r1; \
        }                                                                                      \
    } while (0)
#define BK_RGBA_VAL(Q_, E_) (RUBIX ? bk_rgba_tint_chunk<2>((Q_), (E_), pal_s) : (Q_))
#define BK_RGBA_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")      /* LDS traffic only: BK_LDS_BARRIER */
    uint8_t *mine = buf + threadIdx.x * 16u;
    // SS: NS = the groups this lane averages and stores, ix.iw[0 .. NS) - and ix.iw[NS .. RG) are the ones lane l ^ LPR stores, which
    // this lane gathers its row's half of (rgba_load_idx); RG = 1: both lanes hold the one group, the even row's lane stores it
    constexpr int NS = RG > 1 ? RG / 2 : 1;
    const bool odd = SS && (((threadIdx.x & 63u) / LPR) & 1u);
    const bool storing = RG > 1 || !odd;
    uint32_t cnt[NS];                         // per stored group: the mapped samples of its two quads, 0 .. 4 in bits 0-15 / 16-31
    if (SS && !tile_empty) {
        uint32_t m[RG];
#pragma unroll
        for (int r = 0; r < RG; ++r) {
            const uint32_t a[4] = {ix.iw[r].x & 0xFFFFu, ix.iw[r].x >> 16, ix.iw[r].y & 0xFFFFu, ix.iw[r].y >> 16};
            m[r] = ((a[0] != 0xFFFFu) + (a[1] != 0xFFFFu)) | (uint32_t)((a[2] != 0xFFFFu) + (a[3] != 0xFFFFu)) << 16;
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) cnt[j] = m[j] + bk_ss2_partner<LPR>(m[RG > 1 ? j + NS : j], odd);
    }
    if (f_begin < f_end) {
        BK_RGBA_LUT_REQUEST(0);
        BK_RGBA_LOADS(f_begin, 0);
        if (RUBIX) {
            BK_RGBA_LUT_COMMIT();
            BK_RGBA_BARRIER();                // plane 0's LUT is in pal_s
        }
    }
    for (int f = f_begin; f < f_end; ++f) {
        uint32_t acc[4][RG];                  // SS: [4][NS] in use, the quad sums of the stored groups, two 10-bit fields per (plane, group)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (k0) *reinterpret_cast<uint4 *>(mine) = BK_RGBA_VAL(q0, s0);
            if (NQ > 1 && k1) *reinterpret_cast<uint4 *>(mine + 4096) = BK_RGBA_VAL(q1, s1);
            if (NQ > 2 && k2) *reinterpret_cast<uint4 *>(mine + 8192) = BK_RGBA_VAL(q2, s2);
            if (NQ > 3 && k3) *reinterpret_cast<uint4 *>(mine + 12288) = BK_RGBA_VAL(q3, s3);
            if (NQ == 4) {
                const uint8_t *gl = BK_RGBA_PLANE(f, c);
                for (uint32_t c0 = 1024; c0 < nchunks; c0 += 1024) {      // blocks above what the registers hold: rounds of four loads
                    const uint32_t n = c0 + threadIdx.x;
                    const bool m0 = n < nchunks, m1 = n + 256u < nchunks, m2 = n + 512u < nchunks, m3 = n + 768u < nchunks;
                    const uint32_t a0 = m0 ? blist[n] : 0u, a1 = m1 ? blist[n + 256u] : 0u, a2 = m2 ? blist[n + 512u] : 0u,
                                   a3 = m3 ? blist[n + 768u] : 0u;
                    q0 = *reinterpret_cast<const uint4 *>(gl + BK_CHUNK_OFF(a0));
                    q1 = *reinterpret_cast<const uint4 *>(gl + BK_CHUNK_OFF(a1));
                    q2 = *reinterpret_cast<const uint4 *>(gl + BK_CHUNK_OFF(a2));
                    q3 = *reinterpret_cast<const uint4 *>(gl + BK_CHUNK_OFF(a3));
                    uint8_t *md = mine + (size_t)c0 * 16u;
                    if (m0) *reinterpret_cast<uint4 *>(md) = BK_RGBA_VAL(q0, a0);
                    if (m1) *reinterpret_cast<uint4 *>(md + 4096) = BK_RGBA_VAL(q1, a1);
                    if (m2) *reinterpret_cast<uint4 *>(md + 8192) = BK_RGBA_VAL(q2, a2);
                    if (m3) *reinterpret_cast<uint4 *>(md + 12288) = BK_RGBA_VAL(q3, a3);
                }
            }
            BK_RGBA_BARRIER();                // the plane's chunks are in `buf`
            const bool more = c < 3 || f + 1 < f_end;       // another plane follows this one
            if (c < 3) { BK_RGBA_LUT_REQUEST(c + 1); BK_RGBA_LOADS(f, c + 1); }
            else if (more) { BK_RGBA_LUT_REQUEST(0); BK_RGBA_LOADS(f + 1, 0); }
            if (SS && !tile_empty) {
                uint32_t h[RG];               // this row's halves of the quad sums: pixel 0 + 1 in bits 0-8, pixel 2 + 3 in bits 16-24
#pragma unroll
                for (int r = 0; r < RG; ++r) {
                    const uint32_t a[4] = {ix.iw[r].x & 0xFFFFu, ix.iw[r].x >> 16, ix.iw[r].y & 0xFFFFu, ix.iw[r].y >> 16};
                    uint32_t v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = (fast_store || a[k] != 0xFFFFu) ? buf[a[k]] : 0u;
                    h[r] = (v[0] + v[1]) | ((v[2] + v[3]) << 16);
                }
#pragma unroll
                for (int j = 0; j < NS; ++j) acc[c][j] = h[j] + bk_ss2_partner<LPR>(h[RG > 1 ? j + NS : j], odd);
                if (c == 3 && storing) {
                    // output row (row0 / 2), the block's output pixels start at byte 2 * xb, a group is two of them
                    const int g0 = RG > 1 ? (odd ? 16 : 0) + cx * NS : cx;
                    uint8_t *out = dst + (size_t)f * frame_stride + (size_t)(row0 >> 1) * dst_pitch + (size_t)xb * 2 + (size_t)g0 * 8;
                    if (fast_store) {         // every sample mapped: (sum + 2) >> 2 on both fields at once
                        uint32_t px[2 * NS];
#pragma unroll
                        for (int j = 0; j < NS; ++j) {
                            const uint32_t d0 = ((acc[0][j] + 0x00020002u) >> 2) & 0x00FF00FFu, d1 = ((acc[1][j] + 0x00020002u) >> 2) & 0x00FF00FFu,
                                           d2 = ((acc[2][j] + 0x00020002u) >> 2) & 0x00FF00FFu, d3 = ((acc[3][j] + 0x00020002u) >> 2) & 0x00FF00FFu;
                            const uint32_t t01 = d0 | (d1 << 8), t23 = d2 | (d3 << 8);      // bytes 0, 1 / 2, 3 of output pixel 0 (low half), 1 (high half)
                            px[2 * j] = __builtin_amdgcn_perm(t23, t01, 0x05040100u);
                            px[2 * j + 1] = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
                        }
                        if constexpr (NS == 1) {
                            typedef uint32_t v2u __attribute__((ext_vector_type(2)));
                            v2u v = {px[0], px[1]};
                            __builtin_nontemporal_store(v, reinterpret_cast<v2u *>(out));
                        } else {
                            typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                            v4u v = {px[0], px[1], px[2], px[3]};
                            __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(out));
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < NS; ++j)
#pragma unroll
                            for (int p = 0; p < 2; ++p) {
                                const uint32_t n = (cnt[j] >> (16 * p)) & 0xFFFFu;
                                if (n)
                                    reinterpret_cast<uint32_t *>(out)[2 * j + p] =
                                        bk_ss2_avg((acc[0][j] >> (16 * p)) & 0xFFFFu, n) | (bk_ss2_avg((acc[1][j] >> (16 * p)) & 0xFFFFu, n) << 8) |
                                        (bk_ss2_avg((acc[2][j] >> (16 * p)) & 0xFFFFu, n) << 16) | (bk_ss2_avg((acc[3][j] >> (16 * p)) & 0xFFFFu, n) << 24);
                            }
                    }
                }
            }
            if (!SS && !tile_empty) {
#pragma unroll
                for (int r = 0; r < RG; ++r) {
                    const uint32_t a[4] = {ix.iw[r].x & 0xFFFFu, ix.iw[r].x >> 16, ix.iw[r].y & 0xFFFFu, ix.iw[r].y >> 16};
                    uint32_t v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = (fast_store || a[k] != 0xFFFFu) ? buf[a[k]] : 0u;
                    acc[c][r] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
                }
                if (c == 3) {
                    uint8_t *out = dst + (size_t)f * frame_stride + (size_t)row0 * dst_pitch + (size_t)xb * 4 + (size_t)cx * 16;
#pragma unroll
                    for (int r = 0; r < RG; ++r) {
                        uint32_t px[4];
                        bk_rgba_transpose(acc[0][r], acc[1][r], acc[2][r], acc[3][r], px);
                        if (fast_store) {
                            // non-temporal, as the 8-bit frames: never read back here, L2 stays with the globe lines blocks share
                            typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                            v4u v = {px[0], px[1], px[2], px[3]};
                            __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(out + 16 * LPR * r));
                        } else {
                            const uint32_t a[4] = {ix.iw[r].x & 0xFFFFu, ix.iw[r].x >> 16, ix.iw[r].y & 0xFFFFu, ix.iw[r].y >> 16};
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (a[k] != 0xFFFFu) reinterpret_cast<uint32_t *>(out + 16 * LPR * r)[k] = px[k];
                        }
                    }
                }
            }
            if (more) BK_RGBA_LUT_COMMIT();   // (every wave has passed the barrier above: nobody reads this plane's LUT any more)
            BK_RGBA_BARRIER();                // every wave is done with `buf`
        }
    }
#undef BK_RGBA_VAL
#undef BK_RGBA_LUT_COMMIT
#undef BK_RGBA_LUT_REQUEST
#undef BK_RGBA_BARRIER
#undef BK_RGBA_LOADS
#undef BK_RGBA_PLANE
}

// the LDS addresses of the four-pixel groups this lane takes: group g = r * LPR + cx of its row, which the block map files under lane
// (row's first lane + g / RG), row group g % RG ([blk][wave][RG][64 lanes][4] u16)
// SS: the groups of the head comment's supersampling paragraph - NS = RG / 2 neighbouring groups of this row's own half (the even row's
// lanes own groups 0-15, the odd row's 16-31) in iw[0 .. NS), the same of the other half in iw[NS .. RG); RG = 1: group cx as ever
template <int RG, bool SS>
__device__ __forceinline__ CoopIdx<RG> rgba_load_idx(const uint16_t *__restrict__ idx, int blk, int wave, int lane)
{
    constexpr int LPR = 32 / RG, NS = RG > 1 ? RG / 2 : 1;
    const int first = lane - lane % LPR, cx = lane % LPR, odd = (lane / LPR) & 1;
    CoopIdx<RG> ix;
#pragma unroll
    for (int r = 0; r < RG; ++r) {
        const int g = SS && RG > 1 ? ((r / NS) ^ odd) * 16 + cx * NS + r % NS : r * LPR + cx;
        const size_t slab = (((size_t)blk * 4 + wave) * RG + g % RG) * 256 + (size_t)(first + g / RG) * 4;
        ix.iw[r] = *reinterpret_cast<const uint2 *>(idx + slab);
    }
    return ix;
}

// truecolour frames of a block the staging does not serve: straight from the lensmap, pixel by pixel
// RUBIX: the pixel's tint from the lensmap's tint plane ([rows][W], as coop_slow_frames), its four bytes through the LUTs in device memory
// SS: the even row's lane takes both rows of its 4 * RG pixels, quad by quad, and stores the quads that have a mapped sample
template <int RG, bool RUBIX, bool SS>
__device__ __forceinline__ void rgba_direct_frames(const uint32_t *__restrict__ lmap, const uint8_t *__restrict__ globe, size_t globe_stride,
                                                   int tglobes, int globe0, int f_begin, int f_end, uint8_t *__restrict__ dst, int dst_pitch,
                                                   size_t frame_stride, int W, int rows, int row0, int x,
                                                   const uint8_t *__restrict__ tints, const uint8_t *__restrict__ lut)
{
    if (row0 >= rows) return;
    if (SS) {
        if (row0 & 1) return;
        for (int f = f_begin; f < f_end; ++f) {
            const uint8_t *p0 = globe + (size_t)(4 * ((globe0 + f) % tglobes)) * globe_stride;
            uint32_t *out = reinterpret_cast<uint32_t *>(dst + (size_t)f * frame_stride + (size_t)(row0 >> 1) * dst_pitch + (size_t)x * 2);
            for (int q = 0; q < 2 * RG; ++q) {
                if (x + 2 * q >= W) break;
                uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, n = 0;
                for (int k = 0; k < 4; ++k) {
                    const int sx = x + 2 * q + (k & 1), sy = row0 + (k >> 1);
                    if (sx >= W || sy >= rows) continue;
                    const uint32_t o = lmap[(size_t)sy * W + sx];
                    if (o == BK_NULL_OFFSET) continue;
                    uint32_t b0 = p0[o], b1 = p0[globe_stride + o], b2 = p0[2 * globe_stride + o], b3 = p0[3 * globe_stride + o];
                    if (RUBIX) {
                        const uint32_t t = tints[(size_t)sy * W + sx];
                        if (t < (uint32_t)BK_MAX_PLATES) {
                            const uint8_t *row = lut + t * 256u;
                            b0 = row[b0]; b1 = row[BK_PAL_BYTES + b1]; b2 = row[2 * BK_PAL_BYTES + b2]; b3 = row[3 * BK_PAL_BYTES + b3];
                        }
                    }
                    s0 += b0; s1 += b1; s2 += b2; s3 += b3; ++n;
                }
                if (n) out[q] = bk_ss2_avg(s0, n) | (bk_ss2_avg(s1, n) << 8) | (bk_ss2_avg(s2, n) << 16) | (bk_ss2_avg(s3, n) << 24);
            }
        }
        return;
    }
    for (int f = f_begin; f < f_end; ++f) {
        const uint8_t *p0 = globe + (size_t)(4 * ((globe0 + f) % tglobes)) * globe_stride;
        uint32_t *out = reinterpret_cast<uint32_t *>(dst + (size_t)f * frame_stride + (size_t)row0 * dst_pitch + (size_t)x * 4);
        for (int i = 0; i < 4 * RG; ++i) {
            if (x + i >= W) break;
            const uint32_t o = lmap[(size_t)row0 * W + x + i];
            if (o == BK_NULL_OFFSET) continue;
            uint32_t b0 = p0[o], b1 = p0[globe_stride + o], b2 = p0[2 * globe_stride + o], b3 = p0[3 * globe_stride + o];
            if (RUBIX) {
                const uint32_t t = tints[(size_t)row0 * W + x + i];
                if (t < (uint32_t)BK_MAX_PLATES) {
                    const uint8_t *row = lut + t * 256u;
                    b0 = row[b0]; b1 = row[BK_PAL_BYTES + b1]; b2 = row[2 * BK_PAL_BYTES + b2]; b3 = row[3 * BK_PAL_BYTES + b3];
                }
            }
            out[i] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        }
    }
}

// globe_frames = TRUECOLOUR globes resident (ring slots / 4), frame0 = the first one, nframes / fchunk in truecolour frames; dst =
// pixel (0, first owned row), 4 bytes per pixel.  order, bands: unused (BK_COOP_KERNEL_ARGS is the launchers' one list); tint_t and pal
// are read by the RUBIX instantiations only - there pal = the four planes' LUTs, uint8 [4][BK_MAX_PLATES][256], and the block map is
// the TINTED one.
// (no amdgpu_waves_per_eu: the twelve more accumulator dwords than the 8-bit one-block form put RG = 4 at 77 VGPRs = 6 waves per SIMD;
//  asking for 8 would spill them, and at RG = 4 the staging buffer - 18 KiB and more on real lenses - allows 8 workgroups per CU at best)
template <int RG, bool RUBIX, bool SS>
__device__ __forceinline__ void rgba_workgroup(BK_COOP_KERNEL_ARGS)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    (void)tint_t; (void)pal; (void)order; (void)bands;
    uint8_t *pal_s = smem + lds_buf;                  // RUBIX: one plane's LUT behind the staging buffer (the launch asks for BK_PAL_BYTES more)
    constexpr int N = 1024 * RG;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int blk;
    if (kflags & BK_KF_WGMAP) {                       // bands of equal cost, as apply_coop_once_kernel
        const uint32_t m = wgmap[blockIdx.x];
        if (m == 0xFFFFFFFFu) return;
        blk = (int)m;
    } else {
        const int per = (nblocks + 7) / 8, band = (int)(blockIdx.x & 7);
        const int l = band * per + (int)(blockIdx.x >> 3);
        if (l >= min(nblocks, (band + 1) * per)) return;
        blk = bk_block_at(l, blocks_x, nblocks, kflags);
    }
    const int f_begin = blockIdx.y * fchunk, f_end = min(nframes, f_begin + fchunk);
    // (SS: dst is the half-size frame; its wide stores are 8 bytes per lane for RG = 1 / 2, 16 for RG = 4)
    const bool aligned = ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)dst_pitch | (uintptr_t)frame_stride) & (uintptr_t)(SS && RG < 4 ? 7 : 15)) == 0;
    constexpr int LPR = 32 / RG;                      // a lane's row as in coop_compile_kernel; its pixels of that row: see the head comment
    const int ry = wave * 2 * RG + lane / LPR, cx = lane % LPR;
    const CoopPrefetch<RG> cur = coop_fetch<RUBIX, RG>(hdr, list, blk);
    const uint32_t nchunks = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.h.x);
    const uint32_t flags = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.h.y);
    if (flags & CF_EMPTY) return;
    const int by = blk / blocks_x, bx = blk - by * blocks_x;
    // (x: the lane's 4 * RG CONSECUTIVE pixels, coop_compile_kernel's mapping - used by the direct gather below only, which reads
    //  the lensmap and needs no block-map addresses; the staged path takes the strided groups of the head comment instead)
    const int row0 = by * 8 * RG + ry, x = bx * 128 + cx * 4 * RG;
    const bool tile_all = (flags >> wave) & 1u, tile_empty = (flags >> (4 + wave)) & 1u;
    if ((flags & CF_SLOW) || (int)(nchunks * 16u) > lds_buf) {
        if (!tile_empty)
            rgba_direct_frames<RG, RUBIX, SS>(lmap, globe, globe_stride, globe_frames, frame0, f_begin, f_end, dst, dst_pitch, frame_stride, W, rows,
                                              row0, x, tint_t, pal);
        return;
    }
    const CoopIdx<RG> ix = rgba_load_idx<RG, SS>(idx, blk, wave, lane);
    const bool k0 = threadIdx.x < nchunks, k1 = threadIdx.x + 256u < nchunks, k2 = threadIdx.x + 512u < nchunks, k3 = threadIdx.x + 768u < nchunks;
    const uint32_t s0 = k0 ? cur.c[0] : 0u, s1 = k1 ? cur.c[1] : 0u, s2 = k2 ? cur.c[2] : 0u, s3 = k3 ? cur.c[3] : 0u;
    const uint32_t *bl = list + (size_t)blk * N;
    const bool fast_store = tile_all && aligned;
    const uint32_t nq = (nchunks + 255u) >> 8;
#define BK_RGBA(NQ_) rgba_frames<NQ_, RG, RUBIX, SS>(globe, globe_stride, globe_frames, frame0, f_begin, f_end, dst, dst_pitch, frame_stride, smem, bl, nchunks, \
                                                 s0, s1, s2, s3, k0, k1, k2, k3, ix, fast_store, tile_empty, row0, bx * 128, cx, pal, pal_s)
    if (nq <= 1) BK_RGBA(1);
    else if (nq == 2) BK_RGBA(2);
    else if (nq == 3) BK_RGBA(3);
    else BK_RGBA(4);
#undef BK_RGBA
}
#define BK_COOP_KERNEL_ARG_NAMES                                                                                                    \
    hdr, list, idx, tint_t, lmap, globe, globe_stride, globe_frames, frame0, dst, dst_pitch, frame_stride, W, rows, blocks_x, nblocks, \
    nframes, fchunk, lds_buf, pal, kflags, order, bands, wgmap
template <int RG, bool SS = false>
__global__ __launch_bounds__(256) void apply_coop_rgba_kernel(BK_COOP_KERNEL_ARGS)
{
    rgba_workgroup<RG, false, SS>(BK_COOP_KERNEL_ARG_NAMES);
}
// the tinted launch's kernel (no amdgpu_waves_per_eu either: asked for the plain kernel's 6 waves per SIMD, RG = 4 spills 60 bytes per lane)
template <int RG, bool SS = false>
__global__ __launch_bounds__(256) void apply_coop_rgba_tinted_kernel(BK_COOP_KERNEL_ARGS)
{
    rgba_workgroup<RG, true, SS>(BK_COOP_KERNEL_ARG_NAMES);
}
#undef BK_COOP_KERNEL_ARG_NAMES

// dst = address of pixel (0, row0) of truecolour frame 0, i.e. the first owned row; globe0 / nframes in truecolour globes / frames;
// d_lut != nullptr: the tinted launch (bk_apply_rgba_tinted_device); ss2: the supersampling launch (bk_apply_rgba_ss2_device) - dst is
// then pixel (0, row0 / 2) of the HALF-SIZE frame 0, and everything else about the launch is the same
int launch_apply_rgba(bk_ctx *ctx, int globe0, int nframes, uint8_t *dst, int dst_pitch, size_t frame_stride, const uint8_t *d_lut, bool ss2)
{
    const int rows = ctx->rows();
    if (rows <= 0 || nframes <= 0) return BK_OK;
    const int planes = 4 * nframes;
    const bool rubix = d_lut != nullptr;
    // the plain / the tinted block map, compiled and tuned as for a launch of that many 8-bit frames of that flavour (the tuning launches
    // of a tinted map are 8-bit rubix launches through whatever ctx->pal.d holds: their output is scratch)
    if (int r = ensure_coopmap(ctx, planes, rubix ? 1 : 0)) return r;
    CoopMap *cm = ctx->coopmap;
    if (rubix != cm->tinted) return ctx->fail(BK_E_STATE, "truecolour apply: the block map is not of this launch's flavour (internal)");
    const int nblocks = cm->blocks_x * cm->blocks_y;
    // planes per block visit as an 8-bit launch of that many frames has them; a visit serves whole truecolour frames
    const int fchunk = std::max(1, coop_frames_per_visit(ctx, cm, planes) / 4);
    const int fblocks = (nframes + fchunk - 1) / fchunk;
    const int per = (nblocks + 7) / 8;
    const int lds_buf = coop_launch_lds(ctx, cm);
    // Of the developer ablations (ctx->apply_flags, bk_debug_set_ablation) this kernel knows one: BK_AB_ROW_MAJOR, the row-major walk its
    // bk_block_at call honours.  The others switch parts of the 8-bit kernels this one does not have (forms, DMA staging, the
    // pipelining, stores off ...) and are deliberately not passed on.
    int kflags = ctx->apply_flags & BK_AB_ROW_MAJOR;
    if (coop_wants_wgmap(cm, ctx->apply_flags)) kflags |= BK_KF_WGMAP;
    const dim3 grid((unsigned)(per * 8), (unsigned)fblocks);
    const CoopKernel kernel =
        ss2 ? (rubix ? (cm->rg == 1 ? apply_coop_rgba_tinted_kernel<1, true> : cm->rg == 2 ? apply_coop_rgba_tinted_kernel<2, true> : apply_coop_rgba_tinted_kernel<4, true>)
                     : (cm->rg == 1 ? apply_coop_rgba_kernel<1, true> : cm->rg == 2 ? apply_coop_rgba_kernel<2, true> : apply_coop_rgba_kernel<4, true>))
            : (rubix ? (cm->rg == 1 ? apply_coop_rgba_tinted_kernel<1> : cm->rg == 2 ? apply_coop_rgba_tinted_kernel<2> : apply_coop_rgba_tinted_kernel<4>)
                     : (cm->rg == 1 ? apply_coop_rgba_kernel<1> : cm->rg == 2 ? apply_coop_rgba_kernel<2> : apply_coop_rgba_kernel<4>));
    return coop_launch(kernel, ctx, cm, grid, (size_t)lds_buf + (rubix ? BK_PAL_BYTES : 0), ctx->nframes / 4, globe0, nframes, fchunk, lds_buf, dst,
                       dst_pitch, frame_stride, rubix ? d_lut : ctx->pal.d, kflags);
}
