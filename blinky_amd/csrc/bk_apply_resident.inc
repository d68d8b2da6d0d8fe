// blinky-hip: the RESIDENT single-frame apply (textually included by bk_apply_coop.hip, inside namespace bk).
//
// The engine's real call is one frame per F_RenderView (engine/NQ/fisheye.c:803 -> render_lensmap, 2406-2424).  As a kernel
// launch per frame that moves the whole block map - headers, chunk lists, 2 bytes of LDS address per pixel: 19.6 MB at 4K panini,
// half of the launch's traffic - through the fabric every time: an XCD's L2 does not carry clean lines over a kernel boundary
// (profiles/r03_single_frame_nt_dma.txt).  What keeps the map on the chip is not ending the kernel.
//
// apply_resident_kernel is launched once (bk_apply_resident_begin) and stays on the CUs.  Every workgroup owns a fixed set of
// blocks for the kernel's lifetime and holds what the block map says about its first K of them in REGISTERS - the chunk
// offsets a thread fetches (NQ per block) and its pixels' LDS addresses (the register file is 128 MB per chip: the 4K block map
// is a sixth of it); blocks beyond K, or too large for the register plan, go through the streaming code of the launch-per-frame
// kernel (coop_block).  A frame is a COMMAND: the host writes {sequence number, globe frame, destination, pitch} into a ring in pinned
// host memory; one service wave (the last workgroup's wave 0) polls that ring over PCIe and re-publishes the command in device
// memory (8 copies 4 KiB apart, one per XCD: 2048 pollers on one address would queue on one memory channel); the workers poll
// their copy with relaxed agent-scope loads + s_sleep.  Workgroups never wait for one another: one that finishes frame n starts
// frame n+1 as soon as its command is there, so back-to-back submissions pipeline like the frames of a batch launch.
//
// Visibility without a kernel boundary (MI355X_MICROARCH.md, "Contract"): per-CU L1s are never refreshed by other CUs' stores and
// an agent-scope acquire per workgroup and frame costs more than the frame (1.7 us x 4 at 4 workgroups per CU), so
//  - globe chunks are fetched with non-temporal loads, which bypass L1 (a globe slot may have been rewritten since the last frame
//    that read it; whoever rewrote it - a kernel, a DMA - had finished before the host raised the flag); workgroups with blocks on
//    the plain-load paths (multi-pass, direct gather) pay the acquire;
//  - the frame is stored write-through (`sc1`: coop_gather_store<.., WT = true>), every wave drains its stores (s_waitcnt vmcnt(0)),
//    the workgroup meets at a barrier and one lane raises the workgroup's own flag word (no shared counter: 2048 arrivals on one word
//    take ~25 us); workgroups with blocks on the streaming paths (plain / nt stores) pay a release fence first;
//  - a collector wave (the service workgroup's wave 1) sweeps the flag words - 8 KB - and publishes min(flags) = "every frame up to
//    here is complete" to the host ring, with device timestamps (s_memrealtime) of command-forwarded and frame-complete.
// Nobody can hang: the service wave turns `idle_ticks` without a command into an exit command, workers leave on their own after
// twice that, and the host side (below) relaunches transparently when it finds the kernel gone.

#ifndef BK_RES_RELAY_SLEEP
#define BK_RES_RELAY_SLEEP 8
#endif
#ifndef BK_RES_COLLECT_SLEEP
#define BK_RES_COLLECT_SLEEP 4      /* s_sleep between the collector's sweeps while a frame is out: 16 -> 4 (r6) took 0.45 us off a one-at-a-time frame, 2 gave some back */
#endif
constexpr int BK_RES_RING = 64;                       // command slots (the host keeps at most half of them in flight)
constexpr uint32_t BK_RES_FRAME = 1, BK_RES_EXIT = 2;
constexpr int BK_RES_MAX_COPIES = 256, BK_RES_COPY_WORDS = BK_RES_RING * 8;      // device copies of the ring (2 KiB each): 16 pollers per copy

struct ResHost {                                      // pinned, coherent host memory
    volatile uint32_t cmd[BK_RES_RING][8];            // [0] seq (1-based, written LAST) [1] op [2] globe frame [3] pitch [4,5] dst [6] - [7] seq (written before [0])
    volatile uint32_t completed; uint32_t pad0[15];   // collector -> host: every frame with seq <= completed is in memory
    volatile uint32_t exited; uint32_t pad1[15];      // collector -> host: the kernel has left; commands with seq >= exited were not run
    volatile uint32_t up; uint32_t pad2[15];          // collector -> host: workers that have started
    volatile uint32_t dbg[16];                         // developer counters of workgroup 0: [0] frames, [1] frames that went on without a drain
    volatile uint64_t t_fwd[BK_RES_RING];             // device clock (100 MHz) when the command was re-published
    volatile uint64_t t_done[BK_RES_RING];            // ... when the collector saw the frame complete
};

struct ResArgs {
    const CoopHdr *hdr; const uint32_t *list; const uint16_t *idx; const uint8_t *tint_t; const uint32_t *lmap;
    const uint8_t *globe; size_t globe_stride; int globe_frames;
    int W, rows, blocks_x, nblocks, lds_buf; const uint8_t *pal; int kflags;
    // who does what, planned on the host (res_plan): workgroup b's blocks are assign[b * depth ..], -1 = no more, -2 in the first
    // place = a SLEEPER (it only keeps a place occupied: the other places of the service workgroup's CU); workgroup `service`
    // relays commands and collects flags
    const int *assign; int depth; int service;
    ResHost *rh; uint32_t *ring; uint32_t *wg_done; uint32_t *wg_up; int nwg;          // nwg = the whole grid
    uint32_t *exit_flag; uint32_t idle_ticks;
    int ncopies;                 // copies of the device ring the relay writes; workgroup b polls copy b % ncopies
    // (r5) FRAME STRIDE: a map with fewer blocks than the chip has places (a 270-row stripe, 1080p) is dealt out `stride` times over -
    // the workgroups of group p warp the frames with tickets p + 1, p + 1 + stride, ... - so that pipelined submissions run `stride`
    // frames side by side instead of leaving most of the chip idle.  A workgroup's flag word says "every frame of MINE up to here":
    // it starts at p and is raised to ticket + stride - 1, so min(flags) is still "every frame up to here".
    int stride; const int *phase;
};

// lane `src` of v for the whole wave; src is a constant at every call site in the workers: v_readlane, no address register
__device__ __forceinline__ uint32_t res_lane_bcast(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }

// the last workgroup: wave 0 relays commands host ring -> device ring, wave 1 collects the workers' flags
struct ResService { ResHost *rh; uint32_t *ring, *wg_done, *wg_up; int nwg; uint32_t idle_ticks; int ncopies; int kflags; uint32_t *exit_flag; };
__device__ __noinline__ void res_service(ResHost *rh, uint32_t *ring, uint32_t *wg_done, uint32_t *wg_up, int nwg, uint32_t idle_ticks, int ncopies, int kflags,
                                         uint32_t *exit_flag)
{
    const ResService a = {rh, ring, wg_done, wg_up, nwg, idle_ticks, ncopies, kflags, exit_flag};      // (by value: a reference to the kernel's argument block would force all of it into scratch)
    __shared__ volatile uint32_t s_fwd, s_exit;       // frames forwarded so far / sequence number of the exit command (0 = none yet)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) { s_fwd = 0; s_exit = 0; }
    __syncthreads();
    if (wave == 0) {
        // the relay: one PCIe read fetches the next EIGHT command slots (64 lanes x 4 bytes); every consecutive valid command among
        // them is re-published in one go - all their payload halves, one drain, all their sequence-word halves - so that the
        // relay keeps up with a host that submits faster than a PCIe round trip per frame
        uint32_t seq = 0;
        long long t_last = wall_clock64();
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
        for (;;) {
            const uint32_t slot = (seq + (uint32_t)(lane >> 3)) % BK_RES_RING;
            // (r5) DIRECT submission: the host has written the command into every device copy itself, through the PCIe BAR (posted writes) -
            // the relay is off the frame's path; it watches copy 0 for the time stamps and the idle timer.  Its own exit (nobody has asked for a
            // frame) is NOT written into the copies - the host may be writing that very ticket - but left in the exit word, which the workers
            // look at while they wait; a frame some of them still saw is reported as not run (`exited`) and submitted again by the host
            const bool direct = (a.kflags & BK_KF_DIRECT) != 0;
            uint32_t v = direct ? __hip_atomic_load(a.ring + slot * 8 + (lane & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                : __hip_atomic_load(const_cast<uint32_t *>(&a.rh->cmd[slot][lane & 7]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            int nvalid = 0;
            bool exit_cmd = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (nvalid != j || exit_cmd) break;
                if (res_lane_bcast(v, 8 * j) != seq + 1 + j || res_lane_bcast(v, 8 * j + 7) != seq + 1 + j) break;
                ++nvalid;
                if (res_lane_bcast(v, 8 * j + 1) != BK_RES_FRAME) exit_cmd = true;
            }
            if (nvalid == 0 && (uint64_t)(wall_clock64() - t_last) > (uint64_t)a.idle_ticks) {       // nobody has asked for a frame: leave
                nvalid = 1;
                exit_cmd = true;
                v = lane == 1 ? BK_RES_EXIT : 0u;
            }
            if (nvalid == 0) { if (direct) __builtin_amdgcn_s_sleep(BK_RES_RELAY_SLEEP); else __builtin_amdgcn_s_sleep(4); continue; }
            if (!direct) {
            for (int j = 0; j < nvalid; ++j) {
                const v4u tail = {res_lane_bcast(v, 8 * j + 4), res_lane_bcast(v, 8 * j + 5), res_lane_bcast(v, 8 * j + 6), seq + 1 + j};
                for (int c = lane; c < a.ncopies; c += 64) {
                    uint32_t *dp = a.ring + (size_t)c * BK_RES_COPY_WORDS + ((seq + j) % BK_RES_RING) * 8;
                    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dp + 4), "v"(tail) : "memory");
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (write-through stores: the payloads are in memory before any sequence word)
            for (int j = 0; j < nvalid; ++j) {
                const v4u head = {seq + 1 + j, res_lane_bcast(v, 8 * j + 1), res_lane_bcast(v, 8 * j + 2), res_lane_bcast(v, 8 * j + 3)};
                for (int c = lane; c < a.ncopies; c += 64) {
                    uint32_t *dp = a.ring + (size_t)c * BK_RES_COPY_WORDS + ((seq + j) % BK_RES_RING) * 8;
                    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dp), "v"(head) : "memory");
                }
            }
            }
            if (lane == 0) {
                const uint64_t now = (uint64_t)wall_clock64();
                for (int j = 0; j < nvalid; ++j) a.rh->t_fwd[(seq + j) % BK_RES_RING] = now;
            }
            seq += (uint32_t)nvalid;
            if (exit_cmd) { if (lane == 0) { s_exit = seq; __hip_atomic_store(a.exit_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } break; }      // (the exit command's ticket: workgroups with a frame stride compare their next frame with it)
            if (lane == 0) s_fwd = seq;
            t_last = wall_clock64();
        }
    } else if (wave == 1) {
        uint32_t completed = 0, up = 0;
        int idle_spins = 0;
        for (;;) {
            const uint32_t ex = s_exit;
            const uint32_t frames = ex ? ex - 1 : s_fwd;             // commands that ask for a frame, so far
            bool busy = false;
            if (up < (uint32_t)a.nwg - 1u) {        // (everybody but this workgroup)
                uint32_t n = 0;
                for (int i = lane; i < a.nwg; i += 64) n += __hip_atomic_load(a.wg_up + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
                for (int m = 32; m >= 1; m >>= 1) n += (uint32_t)__shfl_xor((int)n, m);
                if (n != up) { up = n; if (lane == 0) __hip_atomic_store(const_cast<uint32_t *>(&a.rh->up), up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
                busy = true;
            }
            if (completed < frames) {
                // (the flag words as 16-byte device-scope loads, eight per lane in flight: one trip to memory per 2048 workgroups; the
                //  array is padded with 0xFFFFFFFF to a multiple of that)
                uint32_t m = 0xFFFFFFFFu;
                typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                for (int i0 = 0; i0 < a.nwg; i0 += 2048) {
                    const uint32_t *p0 = a.wg_done + i0 + lane * 4;
                    v4u t0, t1, t2, t3, t4, t5, t6, t7;
                    asm volatile("global_load_dwordx4 %0, %8, off sc1\n\tglobal_load_dwordx4 %1, %8, off offset:1024 sc1\n\t"
                                 "global_load_dwordx4 %2, %8, off offset:2048 sc1\n\tglobal_load_dwordx4 %3, %8, off offset:3072 sc1\n\t"
                                 "global_load_dwordx4 %4, %9, off sc1\n\tglobal_load_dwordx4 %5, %9, off offset:1024 sc1\n\t"
                                 "global_load_dwordx4 %6, %9, off offset:2048 sc1\n\tglobal_load_dwordx4 %7, %9, off offset:3072 sc1\n\t"
                                 "s_waitcnt vmcnt(0)"
                                 : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4), "=&v"(t5), "=&v"(t6), "=&v"(t7)
                                 : "v"(p0), "v"(p0 + 1024)
                                 : "memory");
                    const v4u u = {min(min(t0.x, t1.x), min(t2.x, t3.x)), min(min(t0.y, t1.y), min(t2.y, t3.y)), min(min(t0.z, t1.z), min(t2.z, t3.z)),
                                   min(min(t0.w, t1.w), min(t2.w, t3.w))};
                    const v4u w = {min(min(t4.x, t5.x), min(t6.x, t7.x)), min(min(t4.y, t5.y), min(t6.y, t7.y)), min(min(t4.z, t5.z), min(t6.z, t7.z)),
                                   min(min(t4.w, t5.w), min(t6.w, t7.w))};
                    m = min(m, min(min(min(u.x, u.y), min(u.z, u.w)), min(min(w.x, w.y), min(w.z, w.w))));
                }
                for (int s = 32; s >= 1; s >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, s));
                if (m > completed) {
                    if (lane == 0) {
                        const uint64_t now = (uint64_t)wall_clock64();
                        for (uint32_t f = completed; f < m && f < completed + BK_RES_RING; ++f) a.rh->t_done[f % BK_RES_RING] = now;
                        // (r6) NOT a release store: a system-scope release writes this XCD's whole L2 back (buffer_wbl2) before the store - once per
                        // frame, in the XCD the collector happens to run in, whose 248 workers then ran 45 % slower than everybody else's and set the
                        // frame rate (tools/r6_wg_busy.py: mean busy 2.9 us against 2.0, the slow XCD moving with the service workgroup;
                        // profiles/r06_resident_service_xcd.txt).  Nothing of the frame is this wave's to release: the workers' pixels are
                        // write-through stores they drained before raising the flags this wave has just read; this wave's own stores before the
                        // word are the time stamps, in the same pinned host memory - ordered by waiting for them.
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __hip_atomic_store(const_cast<uint32_t *>(&a.rh->completed), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    completed = m;
                }
                busy = true;
            } else if (ex) {
                break;                                                // every frame before the exit command is complete
            }
            idle_spins = busy ? 0 : idle_spins + 1;
            // (the sweeps share a CU with seven workers: a sweep every ~0.5 us is as fine-grained as a frame's flag needs to be seen)
            if (busy) __builtin_amdgcn_s_sleep(BK_RES_COLLECT_SLEEP); else if (idle_spins < 64) __builtin_amdgcn_s_sleep(8); else __builtin_amdgcn_s_sleep(32);
        }
        if (lane == 0) __hip_atomic_store(const_cast<uint32_t *>(&a.rh->exited), s_exit, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// A block outside the register plan AND the staging plan (more than NQ * 256 chunks, more than the staging buffer, or no chunk list
// at all: scrambled tables): its pixels straight from the lensmap, byte gathers from the globe (L1-bypassing), write-through byte
// stores.  Rare by construction - the session's staging buffer is sized for the block map's largest listed block.
template <bool RUBIX, int RG>
__device__ __forceinline__ void res_direct_block(const ResArgs &a, const uint8_t *gl, int blk, uint8_t *dst, int dst_pitch, const uint8_t *pal_s,
                                                 int ry, int cx, int wave, int lane)
{
    const int by = blk / a.blocks_x, bx = blk - by * a.blocks_x;
    int row = by * 8 * RG + ry, x0 = bx * 128 + cx * 4 * RG;
    asm volatile("" : "+v"(row), "+v"(x0));      // (a rare path: nothing of it is to be precomputed and kept in registers across the frame loop)
    if (row >= a.rows) return;
    const __amdgpu_buffer_rsrc_t rd = bk_frame_rsrc(dst);
    (void)wave; (void)lane;
#pragma unroll
    for (int r = 0; r < RG; ++r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xx = x0 + 4 * r + k;
            if (xx >= a.W) continue;
            const uint32_t o = a.lmap[(size_t)row * a.W + xx];
            if (o == BK_NULL_OFFSET) continue;
            uint32_t v = __builtin_nontemporal_load(gl + o);
            if (RUBIX) {              // (the lensmap's own tint plane, [rows][W]: a block that is not staged is not tinted in the staging either)
                const uint32_t tt = a.tint_t[(size_t)row * a.W + xx];
                if (tt < (uint32_t)BK_MAX_PLATES) v = pal_s[tt * 256 + v];
            }
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v, rd, (int)((uint32_t)row * (uint32_t)dst_pitch + (uint32_t)xx), 0, 16);
        }
    }
}

// K blocks of the workgroup live in registers, NQ chunk offsets per thread and block (blocks of up to NQ * 4 KiB); TAIL: the
// workgroup may own more than K blocks - the others' chunk offsets and pixel addresses are fetched again every frame
// (two 128x32 blocks with six chunk offsets each are 12 + 16 registers of plan next to a 24-register landing zone: at 96 registers the
//  offsets went to scratch, and a scratch reload stood in front of every globe load of the frame loop - the thing profiles/r04_resident_apply.txt
//  (4a) describes, back through the side door; four workgroups per CU hold the same 2040 blocks two apiece)
// (rubix, one block: six workgroups per CU are what its SGPRs admit - res_try - so it may have six's registers)
constexpr int res_min_waves(int K, bool TAIL, int RG, int NQ, bool RUBIX) { return TAIL ? (K == 1 ? 5 : 3) : K == 1 ? (RUBIX ? 6 : 8) : K == 2 ? (RG == 4 && NQ == 6 ? 4 : 5) : K * RG <= 16 ? 4 : 3; }
template <bool RUBIX, int RG, int K, int NQ, bool TAIL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(res_min_waves(K, TAIL, RG, NQ, RUBIX), 8))) void apply_resident_kernel(const ResArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t s_cmd[8];
    if ((int)blockIdx.x == a.service) { res_service(a.rh, a.ring, a.wg_done, a.wg_up, a.nwg, a.idle_ticks, a.ncopies, a.kflags, a.exit_flag); return; }
    constexpr int N = 1024 * RG;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int *my = a.assign + (size_t)blockIdx.x * a.depth;      // this workgroup's blocks, for as long as the kernel lives
    if (my[0] == -1) {             // a worker the plan gave nothing (per-XCD rounding): its flag word says "done with everything" from the start
        if (threadIdx.x == 0) __hip_atomic_store(a.wg_up + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (my[0] == -2) {
        // a sleeper: holds one of the other places of the service workgroup's CU (the relay's PCIe polls and the collector's sweeps
        // slowed the seven workers that used to share it by a fifth, and the slowest workgroup sets the frame rate) until the exit flag
        if (threadIdx.x == 0) {
            __hip_atomic_store(a.wg_up + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const long long t0 = wall_clock64();
            while (!__hip_atomic_load(a.exit_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                // (no idle limit of its own short of a minute: the relay raises the flag when it leaves, whatever makes it leave)
                if ((uint64_t)(wall_clock64() - t0) > 6000000000ull) break;
                __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127);
            }
        }
        return;
    }
    const int lds_buf = a.lds_buf;
    uint8_t *pal_s = smem + lds_buf;
    if (RUBIX) {                                   // (the palette is fixed for the session: bk_apply_resident_begin)
        for (int i = threadIdx.x; i < BK_MAX_PLATES * 256; i += 256) pal_s[i] = a.pal[i];
    }
    constexpr int LPR = 32 / RG;                   // same pixel -> lane mapping as coop_compile_kernel
    const int ry = wave * 2 * RG + lane / LPR, cx = lane % LPR;
    const int kflags = a.kflags;

    // The one-block form runs at 64 registers, and at 64 the compiler put two of the four chunk offsets into scratch: a scratch reload and
    // an s_waitcnt vmcnt(0) in front of their loads - the second one waiting for the first chunk to ARRIVE, and both for the previous
    // frame's write-through stores (memory operations complete in order).  They live in LDS instead (3 dwords per thread behind the
    // staging buffer): an LDS read waits for nothing but itself.  (Two were not enough - the third then went to scratch; all four do not
    // fit: 16 + 4 KiB eight times over is 512 bytes more than a CU has.)
    constexpr bool LO = K == 1 && NQ == 4 && !TAIL;
    constexpr int LON = 3;                        // offsets NQ - LON .. NQ - 1 live in LDS
    uint32_t *lo_s = reinterpret_cast<uint32_t *>(smem + lds_buf + (RUBIX ? BK_PAL_BYTES : 0)) + threadIdx.x;      // [LON][256]: a wave's reads are one row
    // (r5) K >= 4: the TABLE forms - a workgroup's blocks beyond three used to have their part of the block map fetched again every
    // frame (8K hammer 38.2 us resident against 36.8 launched, 4K gumby 18.6 against 17.9: VERDICT r4).  The chunk offsets of ALL K blocks
    // now live in LDS behind the staging buffer - 4 bytes per chunk, rows of 256 so that a wave's read is conflict-free - and only the
    // pixel addresses (2 * RG dwords per block) stay in registers: four, six or eight blocks per workgroup, nothing of the block map
    // crossing the fabric per frame.  (Tried first: LDS-DMA into a ring of allocations with the loads of up to four blocks in flight - git history,
    // commit "Resident apply form 2", and profiles/r05_resident_apply.txt: in a CU whose other waves are gathering an LDS-DMA instruction
    // stalls at issue for ~1 us, and the form ran 1.7x slower per block than register staging at equal occupancy.)
    constexpr bool TAB = K >= 4;
    uint32_t *tb = reinterpret_cast<uint32_t *>(smem + lds_buf + (RUBIX ? BK_PAL_BYTES : 0)) + threadIdx.x;
    uint32_t toff[K];                              // where block k's offsets start in the table (dwords)
    int blk[K];
    uint32_t nch[K], flg[K];
    int mode[K];                                   // 0 nothing to do, 1 from registers, 2 direct gather
    uint32_t s[TAB ? 1 : K][NQ];                   // (the table forms keep no offsets in registers)
    CoopIdx<RG> ix[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int mine = k < a.depth ? my[k] : -1;
        const bool have = mine >= 0;
        blk[k] = have ? mine : 0;
        const CoopHdr h = a.hdr[blk[k]];
        nch[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.nchunks);
        flg[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.flags);
        const bool fits = (int)(nch[k] * 16u) <= lds_buf;       // (chunks beyond the NQ a thread keeps in registers: BK_RES_OVERFLOW)
        mode[k] = !have || (flg[k] & CF_EMPTY) ? 0 : (flg[k] & CF_SLOW) || !fits ? 2 : 1;
#pragma unroll
        for (int j = 0; j < NQ; ++j) s[TAB ? 0 : k][j] = 0;
#pragma unroll
        for (int r = 0; r < RG; ++r) ix[k].iw[r] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        toff[k] = k == 0 ? 0u : toff[k > 0 ? k - 1 : 0] + (mode[k > 0 ? k - 1 : 0] == 1 ? ((nch[k > 0 ? k - 1 : 0] < (uint32_t)NQ * 256u ? nch[k > 0 ? k - 1 : 0] : (uint32_t)NQ * 256u) + 255u) & ~255u : 0u);
        if (mode[k] == 1) {
            const uint32_t *bl = a.list + (size_t)blk[k] * N;
            if (TAB) {
#pragma unroll
                for (int j = 0; j < NQ; ++j) if (256u * j < nch[k]) tb[toff[k] + 256u * j] = threadIdx.x + 256u * j < nch[k] ? bl[threadIdx.x + 256u * j] : 0u;
            } else {
#pragma unroll
                for (int j = 0; j < NQ; ++j) s[TAB ? 0 : k][j] = threadIdx.x + 256u * j < nch[k] ? bl[threadIdx.x + 256u * j] : 0u;
            }
            ix[k] = coop_load_idx<RUBIX, RG>(a.idx, a.tint_t, blk[k], wave, lane);
        }
        if (LO) {
#pragma unroll
            for (int j = NQ - LON; j < NQ; ++j) { lo_s[256 * (j - (NQ - LON))] = s[TAB ? 0 : k][j]; s[TAB ? 0 : k][j] = 0u; }
        }
    }
    if (threadIdx.x == 0) __hip_atomic_store(a.wg_up + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();                               // (the palette)

    typedef uint32_t bk_v4u __attribute__((ext_vector_type(4)));
    __shared__ uint32_t s_next[8];
    // the first / last block in registers with work; a workgroup whose blocks are all of that kind runs the frames as ONE stream of
    // blocks: the next frame's first chunks are requested before this frame's last gather, and a frame's flag is raised two
    // staging barriers after its last store was issued (below) - no drain, no poll, no first-load latency between pipelined frames
    int first = K, last = -1;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) if (mode[k] == 1) first = k;
#pragma unroll
    for (int k = 0; k < K; ++k) if (mode[k] == 1) last = k;
    bool stream_ok = first < K && !(kflags & BK_RF_SINGLE_FRAMES);   // (developer bit: every frame on its own)
#pragma unroll
    for (int k = 0; k < K; ++k) if (mode[k] == 2) stream_ok = false;
    if (TAIL && a.depth > K && my[K] >= 0) stream_ok = false;

    const uint32_t *my_ring = a.ring + (size_t)(blockIdx.x % (uint32_t)a.ncopies) * BK_RES_COPY_WORDS;
    uint32_t seq = 0;                              // frames this workgroup has done; its frame number j has ticket BK_RES_T(j)
    const uint32_t stride = (uint32_t)a.stride, phase = a.phase ? (uint32_t)a.phase[blockIdx.x] : 0u;
#define BK_RES_T(J_) (phase + 1u + stride * (J_))
    uint32_t pend1 = 0, pend2 = 0;                 // frames whose stores are all issued: ended 0 / 1 staging barriers ago
    uint32_t n_streamed = 0;                       // (developer statistic) frames that went on into the next without a drain
    uint32_t busy_ticks = 0;                       // (developer statistic, BK_RF_WG_TIMING) 100 MHz ticks spent inside frames
    bool have = false;                             // the command of frame seq + 1 is decoded and its first chunks are on their way
    uint32_t peek = 0;                             // wave 0, lanes 0..7: what slot seq + 2 held when frame seq + 1 began
    const uint8_t *gl = a.globe;
    const size_t gl_bytes = a.globe_stride < 0x7FFFFFFFull ? a.globe_stride : 0x7FFFFFFFull;
    uint8_t *dst = nullptr;
    int dst_pitch = 0;
    bool aligned = false, aligned4 = false;        // the frame's address and pitch: multiples of a lane's 4 * RG pixels / of 4
    uint4 q[NQ];
    // a command's words, wave-uniform (SGPRs): LDS hands them back per lane
#define BK_RES_CMD(BUF_, I_) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(BUF_)[I_]))
    // globe chunks by BUFFER loads: the frame's base in a resource descriptor (SGPRs), the chunk's 32-bit offset straight from the
    // thread's register - no 64-bit addresses in VGPRs (with them the 64-register form spilled the offsets and every load waited
    // for the scratch reload of its address: four dependent trips to memory per block); aux 2 = nt: L1 is bypassed
#define BK_RES_RSRC(GL_) __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(GL_), 0, (int)gl_bytes, 0x00020000)
/* (r6) The offsets that live in LDS (LO) are ALL read before the first load goes out.  Read one by one inside the loads' conditionals,   \
   the compiler put each ds_read's result into the first register of the chunk it addresses (v14 of v[14:17]) and, unable to prove that    \
   no earlier load into that register was still in flight, an s_waitcnt vmcnt(0) in front of it - which also waited for the load issued   \
   ten instructions before: a block's second and third chunk per thread were DEPENDENT trips to memory.  Busy time per frame by chunks of  \
   the block, 4K panini: <= 256: 2.0-2.3 us, 257-512: 2.2-2.8, above 512: 3.9-4.0 - a staircase (profiles/r06_resident_service_xcd.txt). */ \
#define BK_RES_ISSUE(RS_, S_, NCH_)                                                                                     \
    do {                                                                                                                \
        uint32_t o_[NQ];                                                                                                \
        _Pragma("unroll") for (int j = 0; j < NQ; ++j) o_[j] = LO && j >= NQ - LON ? lo_s[256 * (j - (NQ - LON))] : (S_)[j]; \
        if (LO) { _Pragma("unroll") for (int j = NQ - LON; j < NQ; ++j) asm volatile("" : "+v"(o_[j])); }               \
        _Pragma("unroll") for (int j = 0; j < NQ; ++j)                                                                  \
            if (threadIdx.x + 256u * j < (NCH_)) {                                                                      \
                const bk_v4u t_ = __builtin_amdgcn_raw_buffer_load_b128((RS_), (int)BK_CHUNK_OFF(o_[j]), 0, 2);         \
                q[j] = make_uint4(t_.x, t_.y, t_.z, t_.w);                                                              \
            }                                                                                                           \
    } while (0)
    /* the same for block KK_ of a table form: its offsets out of LDS (all NQ reads first, then the loads) */
#define BK_RES_ISSUE_K(RS_, KK_)                                                                                        \
    do {                                                                                                                \
        if (TAB) {                                                                                                      \
            uint32_t o_[NQ];                                                                                            \
            _Pragma("unroll") for (int j = 0; j < NQ; ++j) o_[j] = 256u * j < nch[KK_] ? tb[toff[KK_] + 256u * j] : 0u; \
            _Pragma("unroll") for (int j = 0; j < NQ; ++j)                                                              \
                if (threadIdx.x + 256u * j < nch[KK_]) {                                                                \
                    const bk_v4u t_ = __builtin_amdgcn_raw_buffer_load_b128((RS_), (int)BK_CHUNK_OFF(o_[j]), 0, 2);     \
                    q[j] = make_uint4(t_.x, t_.y, t_.z, t_.w);                                                          \
                }                                                                                                       \
        } else { BK_RES_ISSUE(RS_, s[TAB ? 0 : KK_], nch[KK_]); }                                                       \
    } while (0)
    /* (rubix: a classed chunk goes through its palette row on the way - bk_tint_chunk; E_(j) = the chunk's list entry) */                \
#define BK_RES_TO_LDS(NCH_, E_)                                                                                         \
    _Pragma("unroll") for (int j = 0; j < NQ; ++j)                                                                      \
        if (threadIdx.x + 256u * j < (NCH_)) *reinterpret_cast<uint4 *>(smem + threadIdx.x * 16u + 4096u * j) = BK_CHUNK_VAL(q[j], (E_));
    /* (list entry j of register / table block KK_, `j` being BK_RES_TO_LDS's loop variable) */
#define BK_RES_ENTRY_K(KK_) (TAB ? tb[toff[KK_] + 256u * j] : (LO && j >= NQ - LON ? lo_s[256 * (j - (NQ - LON))] : s[TAB ? 0 : KK_][j]))
    // a block with more chunks than the register plan covers: the rest of its list from memory, then those chunks, every frame - two
    // dependent trips to memory, a straggler (the planner prices it).  Tried: fetching the next two list entries with the block's
    // own chunks, so that the extra chunks cost one trip - the two registers and the code around them pushed every form over its
    // register budget (42-148 scratch instructions in the frame loop); an eight-chunk plan needs 128-168 registers and a grid too
    // small to hold such maps.  Maps with blocks above 1536 chunks (4K quincuncial: 120 of 2430) keep the slow path.
#define BK_RES_OVERFLOW(NCH_, BLK_)                                                                                     \
    for (uint32_t c_ = NQ * 256u + threadIdx.x; c_ < (NCH_); c_ += 256u) {                                              \
        const uint32_t e_ = a.list[(size_t)(BLK_) * N + c_];                                                            \
        const bk_v4u t_ = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)BK_CHUNK_OFF(e_), 0, 2);                       \
        *reinterpret_cast<uint4 *>(smem + (size_t)c_ * 16u) = BK_CHUNK_VAL(make_uint4(t_.x, t_.y, t_.z, t_.w), e_);     \
    }
#define BK_RES_GATHER(IX_, FLG_, BLK_)                                                                                  \
    do {                                                                                                                \
        const bool tile_all_ = ((FLG_) >> wave) & 1u, tile_empty_ = ((FLG_) >> (4 + wave)) & 1u;                        \
        if (!tile_empty_) {                                                                                             \
            const int by_ = (BLK_) / a.blocks_x, bx_ = (BLK_) - by_ * a.blocks_x;                                       \
            coop_gather_store<RUBIX, RG, true>(smem, IX_, tile_all_ && aligned, pal_s, dst, 0, dst_pitch, 0, by_ * 8 * RG + ry, \
                                               bx_ * 128 + cx * 4 * RG, kflags | (aligned4 ? BK_KF_ALIGNED4 : 0) | (aligned ? BK_KF_ALIGNED16 : 0)); \
        }                                                                                                               \
    } while (0)
#define BK_RES_RAISE(SEQ_) __hip_atomic_store(a.wg_done + blockIdx.x, (SEQ_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
    // (direct submission: the copies are written by the HOST - system scope; relayed: by another XCD's wave - device scope)
#define BK_RES_PEEK(SEQ_)  (lane < 8 ? ((kflags & BK_KF_DIRECT) ? __hip_atomic_load(my_ring + ((SEQ_) % BK_RES_RING) * 8 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) \
                                                                  : __hip_atomic_load(my_ring + ((SEQ_) % BK_RES_RING) * 8 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0u)

    for (;;) {
        if (!have) {
            // ---- wait for the command of frame seq + 1
            if (wave == 0) {
                const long long t0 = wall_clock64();
                uint32_t v = 0;
                for (int spins = 0;; ++spins) {
                    v = BK_RES_PEEK(BK_RES_T(seq) - 1u);
                    if (res_lane_bcast(v, 0) == BK_RES_T(seq) && res_lane_bcast(v, 7) == BK_RES_T(seq)) break;
                    // (with a frame stride the exit command's ticket need not be one of this workgroup's: the relay leaves it in the exit word)
                    const uint32_t ex = (stride > 1u || (kflags & BK_KF_DIRECT)) && spins > 8 ? __hip_atomic_load(a.exit_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                    if (ex && ex <= BK_RES_T(seq)) { v = lane == 1 ? BK_RES_EXIT : 0u; break; }
                    if (spins > 64 && (uint64_t)(wall_clock64() - t0) > 2ull * a.idle_ticks + 100000ull) { v = lane == 1 ? BK_RES_EXIT : 0u; break; }
                    if (spins < 256) __builtin_amdgcn_s_sleep(2); else __builtin_amdgcn_s_sleep(32);
                }
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) s_cmd[i] = res_lane_bcast(v, i);
                }
            }
            __syncthreads();
            if (BK_RES_CMD(s_cmd, 1) != BK_RES_FRAME) break;
            gl = a.globe + (size_t)(BK_RES_CMD(s_cmd, 2) % (uint32_t)a.globe_frames) * a.globe_stride;
            dst_pitch = (int)BK_RES_CMD(s_cmd, 3);
            dst = reinterpret_cast<uint8_t *>((uintptr_t)BK_RES_CMD(s_cmd, 4) | ((uintptr_t)BK_RES_CMD(s_cmd, 5) << 32));
            aligned = ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)dst_pitch) & (uintptr_t)(4 * RG - 1)) == 0;
            aligned4 = ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)dst_pitch) & (uintptr_t)3) == 0;
            {
                const __amdgpu_buffer_rsrc_t rs0 = BK_RES_RSRC(gl);
#pragma unroll
                for (int k = 0; k < K; ++k) if (k == first) { BK_RES_ISSUE_K(rs0, k); }
            }
            if (stream_ok && wave == 0) peek = BK_RES_PEEK(BK_RES_T(seq + 1u) - 1u);
        }
        have = false;
        const long long t_frame0 = (kflags & BK_RF_WG_TIMING) ? wall_clock64() : 0;      // (developer bit: time every workgroup's frames)
        const __amdgpu_buffer_rsrc_t rs = BK_RES_RSRC(gl);
        const uint8_t *gl_n = gl;                   // the frame after this one, once its command has been seen (stream_ok only)
        uint8_t *dst_n = dst;
        int pitch_n = dst_pitch;

        // ---- the blocks in registers: block k+1's chunks are in flight while block k is gathered
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (mode[k] == 2) res_direct_block<RUBIX, RG>(a, gl, blk[k], dst, dst_pitch, pal_s, ry, cx, wave, lane);
            if (mode[k] != 1) continue;
            BK_RES_TO_LDS(nch[k], BK_RES_ENTRY_K(k));
            BK_RES_OVERFLOW(nch[k], blk[k]);
            if (stream_ok && k == last && wave == 0) {
                const uint32_t p0 = res_lane_bcast(peek, 0), p1 = res_lane_bcast(peek, 1), p2 = res_lane_bcast(peek, 2), p3 = res_lane_bcast(peek, 3),
                               p4 = res_lane_bcast(peek, 4), p5 = res_lane_bcast(peek, 5), p7 = res_lane_bcast(peek, 7);
                if (lane == 0) { s_next[0] = p0; s_next[1] = p1; s_next[2] = p2; s_next[3] = p3; s_next[4] = p4; s_next[5] = p5; s_next[7] = p7; }
            }
            BK_LDS_BARRIER();                      // the block's chunks are in LDS
            // every wave has by now waited for loads it issued after the last stores of the frame in pend2 (in-order return): its
            // flag can go up - AFTER the next loads have been issued (below): a 4-byte write-through store takes its time to be
            // acknowledged, and memory operations complete in order - in front of the loads it would be waited for with them
            const uint32_t raise_now = pend2;
            pend2 = pend1;
            pend1 = 0;
            if (k != last) {
                int nxt = K;                       // the next register block with work: its loads go out before this gather
#pragma unroll
                for (int k2 = K - 1; k2 > k; --k2) if (mode[k2] == 1) nxt = k2;
#pragma unroll
                for (int k2 = 0; k2 < K; ++k2) if (k2 > k && k2 == nxt) { BK_RES_ISSUE_K(rs, k2); }
            } else if (stream_ok) {
                // the frame's last block: is the next frame's command there already?  Then its first chunks go out now
                const uint32_t n0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_next[0]), n1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_next[1]),
                               n7 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_next[7]);
                if (n0 == BK_RES_T(seq + 1u) && n7 == BK_RES_T(seq + 1u) && n1 == BK_RES_FRAME) {
                    have = true;
                    gl_n = a.globe + (size_t)(BK_RES_CMD(s_next, 2) % (uint32_t)a.globe_frames) * a.globe_stride;
                    pitch_n = (int)BK_RES_CMD(s_next, 3);
                    dst_n = reinterpret_cast<uint8_t *>((uintptr_t)BK_RES_CMD(s_next, 4) | ((uintptr_t)BK_RES_CMD(s_next, 5) << 32));
                    const __amdgpu_buffer_rsrc_t rs_n = BK_RES_RSRC(gl_n);
#pragma unroll
                    for (int k2 = 0; k2 < K; ++k2) if (k2 == first) { BK_RES_ISSUE_K(rs_n, k2); }
                    if (wave == 0) peek = BK_RES_PEEK(BK_RES_T(seq + 2u) - 1u);
                }
            }
            if (raise_now && threadIdx.x == 0) BK_RES_RAISE(raise_now);
            BK_RES_GATHER(ix[k], flg[k], blk[k]);
            BK_LDS_BARRIER();                      // every wave is done with the buffer
        }

        // ---- blocks beyond the K in registers: what the block map says about them is fetched again (as the launch-per-frame kernel does)
        if (TAIL) {
            for (int t = K; t < a.depth; ++t) {
                const int b = my[t];
                if (b < 0) break;
                const CoopHdr h = a.hdr[b];
                const uint32_t nc = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.nchunks), fl = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.flags);
                if (fl & CF_EMPTY) continue;
                if ((fl & CF_SLOW) || (int)(nc * 16u) > lds_buf) {
                    res_direct_block<RUBIX, RG>(a, gl, b, dst, dst_pitch, pal_s, ry, cx, wave, lane);
                    continue;
                }
                const uint32_t *bl = a.list + (size_t)b * N;
                uint32_t st[NQ];
#pragma unroll
                for (int j = 0; j < NQ; ++j) st[j] = threadIdx.x + 256u * j < nc ? bl[threadIdx.x + 256u * j] : 0u;
                const CoopIdx<RG> ixt = coop_load_idx<RUBIX, RG>(a.idx, a.tint_t, b, wave, lane);
                BK_RES_ISSUE(rs, st, nc);
                BK_RES_TO_LDS(nc, st[j]);
                BK_RES_OVERFLOW(nc, b);
                BK_LDS_BARRIER();
                BK_RES_GATHER(ixt, fl, b);
                BK_LDS_BARRIER();
            }
        }

        // ---- the end of frame seq + 1
        n_streamed += have ? 1u : 0u;
        if (kflags & BK_RF_WG_TIMING) busy_ticks += (uint32_t)(wall_clock64() - t_frame0);
        if (have) {
            pend1 = BK_RES_T(seq) + stride - 1u;   // its flag is raised two staging barriers from here
            gl = gl_n; dst = dst_n; dst_pitch = pitch_n;
            aligned = ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)dst_pitch) & (uintptr_t)(4 * RG - 1)) == 0;
            aligned4 = ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)dst_pitch) & (uintptr_t)3) == 0;
        } else {
            // nothing to go on with: publish now - every store above is write-through, every wave drains its own
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) BK_RES_RAISE(BK_RES_T(seq) + stride - 1u);
            pend1 = pend2 = 0;
        }
        ++seq;
    }
    if (threadIdx.x == 0) a.wg_up[blockIdx.x] = 0x80000000u | ((kflags & BK_RF_WG_TIMING) ? busy_ticks : n_streamed);       // (read by resident_stop for bk_apply_resident_info)
#undef BK_RES_ISSUE
#undef BK_RES_ISSUE_K
#undef BK_RES_T
#undef BK_RES_RSRC
#undef BK_RES_TO_LDS
#undef BK_RES_ENTRY_K
#undef BK_RES_OVERFLOW
#undef BK_RES_GATHER
#undef BK_RES_RAISE
#undef BK_RES_PEEK
#undef BK_RES_CMD
}

// ---------------------------------------------------------------------------------------------
// host side of the resident apply
// ---------------------------------------------------------------------------------------------
struct Resident {
    hipStream_t stream = nullptr;      // the kernel's own non-blocking stream
    ResHost *h = nullptr;              // pinned
    uint32_t *d_ring = nullptr, *d_done = nullptr, *d_up = nullptr;
    int *d_assign = nullptr;           // the plan: every workgroup's blocks
    uint8_t *d_pal = nullptr;          // the session's OWN copy of the tint LUTs (ctx->pal.d belongs to whoever applied last)
    int *d_phase = nullptr;            // every workgroup's frame phase (frame stride, r5)
    int cap_phase = 0;                 // ints allocated behind d_phase
    int stride = 1;                    // frame stride of the running session (r5)
    bool direct = false;               // commands are written into the device copies by the host itself (large BAR, r5)
    int ncopies = 1;                   // device copies of the command ring of the running session
    uint64_t lost_lo = 1, lost_hi = 0; // tickets [lost_lo, lost_hi] were dropped unrendered (the session could not be resumed): wait says so
    size_t cap_assign = 0;
    int depth = 1;                     // blocks per workgroup, at most
    int cap_wg = 0;                    // allocated flag words
    bool running = false;              // a kernel is (or may still be) on the device
    bool rubix = false;
    bool yielded = false;              // the running form did not leave the reserved places free (bk_set_resident_share: it fits too few times on a CU)
    uint32_t next_seq = 0;             // commands written to the ring since the launch
    uint64_t base = 0;                 // ticket of the launch's first command - 1
    int nwg = 0, K = 0, NQ = 0, rg = 0, per_cu = 0;
    double idle_ms = 200.0;
    int shrink = 0;                    // workgroups per CU to give up (grows when a launch did not become fully resident)
    struct Pending { uint32_t frame; int pitch; uint64_t dst; };
    std::vector<Pending> pending;      // commands of this launch that are not known complete, oldest first (for re-submission)
    uint64_t first_pending = 1;        // ticket of pending[0]
    uint64_t launches = 0;
    double last_gpu_us = 0;
    int streamed_argmax = 0, streamed_many = 0;
    std::vector<int> plan_assign;       // (developer statistics)
    std::vector<uint32_t> plan_hdr_chunks, plan_lines;
    int streamed_min = 0, streamed_med = 0, streamed_max = 0;      // of the last session that was ended: frames a workgroup ran on into the next
};

void resident_free(bk_ctx *ctx);

static inline uint64_t res_now_ns()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

static void res_write_cmd(Resident *R, uint32_t seq, uint32_t op, uint32_t frame, int pitch, uint64_t dst)
{
    if (R->direct) {
        // straight into every device copy of the ring through the BAR: posted writes, no PCIe read anywhere on the way to the workers
        // (the relay's poll of the host ring was a round trip per command: profiles/r05_resident_apply.txt (2), doorbell).  Payload
        // words first, a store fence, then the two sequence words a reader checks.
        const uint32_t slot = (seq - 1) % BK_RES_RING;
        // one pass per copy: the 32 bytes of a slot leave the CPU's write-combining buffer as one posted write, and a reader takes the
        // command only when BOTH its first and its last word carry the ticket (a slot is 32-byte aligned: whatever granularity the
        // write arrives in, words 1-3 travel with word 0 and words 4-6 with word 7).  Two passes with a fence in between cost twice
        // the buffer flushes: 0.62 us of host time per frame with eight copies, which is what a 270-row stripe's frame takes.
        for (int k = 0; k < R->ncopies; ++k) {
            volatile uint32_t *c = R->d_ring + (size_t)k * BK_RES_COPY_WORDS + slot * 8;
            c[0] = seq; c[1] = op; c[2] = frame; c[3] = (uint32_t)pitch; c[4] = (uint32_t)dst; c[5] = (uint32_t)(dst >> 32); c[6] = 0; c[7] = seq;
        }
#if defined(__x86_64__)
        __builtin_ia32_sfence();
#else
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
        return;
    }
    volatile uint32_t *c = R->h->cmd[(seq - 1) % BK_RES_RING];
    c[1] = op; c[2] = frame; c[3] = (uint32_t)pitch; c[4] = (uint32_t)dst; c[5] = (uint32_t)(dst >> 32); c[6] = 0;
    __atomic_thread_fence(__ATOMIC_RELEASE);
    c[7] = seq;
    __atomic_thread_fence(__ATOMIC_RELEASE);
    c[0] = seq;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
}

// the kernel has left or is told to: wait for it; afterwards nothing of this launch is on the device
static int res_drain(bk_ctx *ctx, Resident *R, bool tell)
{
    if (!R->running) return BK_OK;
    if (tell && !R->h->exited && R->next_seq - R->h->completed < (uint32_t)BK_RES_RING - 1) res_write_cmd(R, ++R->next_seq, BK_RES_EXIT, 0, 0, 0);
    BK_HIP(ctx, hipStreamSynchronize(R->stream));
    R->running = false;
    return BK_OK;
}

template <bool RUBIX, int RG, int K, int NQ, bool TAIL>
static int res_try(bk_ctx *ctx, Resident *R, const ResArgs &a, size_t shmem, bool launch, int *places)
{
    int occ = 0;
    if (shmem > 65536) BK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(apply_resident_kernel<RUBIX, RG, K, NQ, TAIL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    BK_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, apply_resident_kernel<RUBIX, RG, K, NQ, TAIL>, 256, shmem));
    // (the tinted one-block form needs 94 SGPRs where the plain one needs 78: with the hardware's own that is the next allocation granule,
    //  and a SIMD then holds six such waves, not the seven the occupancy API reports from registers and LDS - measured: the seventh
    //  workgroup of every CU never started, and the session began with a relaunch)
    if (RUBIX && K == 1 && occ > 6) occ = 6;
    occ -= R->shrink;
    if (occ > 8) occ = 8;
    // bk_set_resident_share: `reserve` slots of every CU stay free, the rest is split between `parts` contexts of this device
    // (a form that fits only a few times on a CU - 64 KiB of staging for a scrambled table - and a reserve as large: the reserve yields
    //  before a context goes without a place; what such a workgroup leaves of a CU's registers and LDS is room for other kernels anyway)
    {
        const int parts = std::max(1, ctx->res_parts);
        int avail = occ - ctx->res_reserve;
        R->yielded = avail < parts;                     // (the form launched last decides: resident_leaves_room)
        if (avail < parts) avail = std::min(occ, parts);
        occ = avail / parts;
    }
    *places = occ > 0 ? occ * ctx->num_cus : 0;
    if (!launch) return BK_OK;
    hipLaunchKernelGGL((apply_resident_kernel<RUBIX, RG, K, NQ, TAIL>), dim3((unsigned)a.nwg), dim3(256), shmem, R->stream, a);
    BK_HIP(ctx, hipGetLastError());
    return BK_OK;
}

// the kernel variants: K = 1 / 2 / 3 hold every block of the map in registers (the host only picks them when that is so), K = 4
// stands for "3 in registers and as many more as it takes, fetched per frame" (TAIL); rubix (r5: tinted in the staging, bk_tint_chunk) takes the same register forms
template <int RG, bool RBX>
static int res_variant(bk_ctx *ctx, Resident *R, const ResArgs &a, size_t shmem, int K, int nq, bool launch, int *places)
{
    // (64 registers: four chunks per thread is what fits - and three of the four offsets only in LDS, `LO` below: a map
    //  that takes this form has no block above 1024 chunks, so the staging buffer is 16 KiB at most and 3 KiB more still let eight
    //  workgroups share a CU)
    if (K == 1) return res_try<RBX, RG, 1, 4, false>(ctx, R, a, shmem + 3072, launch, places);
#define BK_RES_NQ(KV, TAILV) (nq == 6 ? res_try<RBX, RG, KV, 6, TAILV>(ctx, R, a, shmem, launch, places)   \
                                      : res_try<RBX, RG, KV, 4, TAILV>(ctx, R, a, shmem, launch, places))
    if (K == 2) return BK_RES_NQ(2, false);
    if (K == 3) return BK_RES_NQ(3, false);
    if constexpr (!RBX) {                                 // (rubix - a debugging view - has the register forms and the tail, not the table forms)
        if (K == 4) return BK_RES_NQ(4, false);           // 4 / 6 / 8: the table forms (chunk offsets in LDS)
        if (K == 6) return BK_RES_NQ(6, false);
        if (K == 8) return BK_RES_NQ(8, false);
        if (K == 10) return BK_RES_NQ(8, true);           // eight in the table, the rest fetched per frame
    }
    return BK_RES_NQ(3, true);                            // 9: three in registers, the rest fetched per frame
#undef BK_RES_NQ
}
static int res_variant_rg(bk_ctx *ctx, Resident *R, int rg, const ResArgs &a, size_t shmem, int K, int nq, bool launch, int *places)
{
    if (R->rubix)
        return rg == 1 ? res_variant<1, true>(ctx, R, a, shmem, K, nq, launch, places) : rg == 2 ? res_variant<2, true>(ctx, R, a, shmem, K, nq, launch, places)
                                                                                                   : res_variant<4, true>(ctx, R, a, shmem, K, nq, launch, places);
    return rg == 1 ? res_variant<1, false>(ctx, R, a, shmem, K, nq, launch, places) : rg == 2 ? res_variant<2, false>(ctx, R, a, shmem, K, nq, launch, places)
                                                                                                : res_variant<4, false>(ctx, R, a, shmem, K, nq, launch, places);
}

// Who does what - which workgroup warps which blocks in which frame phase - and which of the forms above serves a block map is decided in
// bk_resident_plan.cpp, from plain values: what follows reads the map back, asks there, and launches what it is told.
struct ResMapHost { std::vector<uint32_t> nchunks, order, lines; };      // per block: chunks; the live blocks in walk order; per block: cost in lines

static int res_read_map(bk_ctx *ctx, const CoopMap *cm, ResMapHost *m)
{
    const int nblocks = cm->blocks_x * cm->blocks_y;
    uint32_t bands[9];
    std::vector<CoopHdr> hdr((size_t)nblocks);
    BK_HIP(ctx, hipMemcpyAsync(bands, cm->d_bands, sizeof bands, hipMemcpyDeviceToHost, ctx->stream));
    BK_HIP(ctx, hipMemcpyAsync(hdr.data(), cm->d_hdr, hdr.size() * sizeof(CoopHdr), hipMemcpyDeviceToHost, ctx->stream));
    BK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (block map, palette upload, whatever filled the globes: done before the kernel starts)
    m->order.resize((size_t)bands[8]);
    if (bands[8]) BK_HIP(ctx, hipMemcpy(m->order.data(), cm->d_order, m->order.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    m->lines.resize((size_t)nblocks);                    // what the block map's compile counted per block: 128-byte lines staged + a share per pixel + a constant
    BK_HIP(ctx, hipMemcpy(m->lines.data(), cm->d_cost, m->lines.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    m->nchunks.resize((size_t)nblocks);
    for (int i = 0; i < nblocks; ++i) m->nchunks[(size_t)i] = hdr[(size_t)i].nchunks;
    return BK_OK;
}

// form, grid, stride and plan for the map (res_choose); how many workgroups of a form the device holds is the occupancy API's to say
static int res_choose_form(bk_ctx *ctx, Resident *R, const CoopMap *cm, const ResMapHost &m, size_t staging, bool may_grow, ResChoice *c)
{
    ResChoiceIn in;
    in.max_chunks = cm->stats[CS_MAX_CHUNKS]; in.rg = cm->rg; in.tinted = R->rubix;
    in.no_one_block = (ctx->apply_flags & BK_RF_NO_ONE_BLOCK) != 0; in.no_tables = (ctx->apply_flags & BK_RF_NO_TABLES) != 0; in.no_stride = (ctx->apply_flags & BK_RF_NO_STRIDE) != 0;
    in.may_grow = may_grow; in.ncu = ctx->res_parts > 1 ? RES_NO_SLEEPERS : ctx->num_cus; in.staging_bytes = staging;
    int rc = BK_OK;                                      // (of the first question that failed: nothing is asked after it)
    *c = res_choose(m.nchunks, m.order, in, [&](int form, size_t shmem) {
        int places = 0;
        if (rc == BK_OK) rc = res_variant_rg(ctx, R, cm->rg, ResArgs{}, shmem, form, res_nq(in.max_chunks), false, &places);
        return rc == BK_OK ? places : 0;
    });
    return rc;
}

// the two developer prints (g_debug.print_model): the plan before the launch, the laggards after the session
static void res_print_plan(const ResMapHost &m, const ResChoice &c, uint32_t max_chunks, int lds_buf)
{
    const ResPlan &plan = c.plan;
    int big = 0, big4 = 0;
    for (uint32_t b : m.order) { big += m.nchunks[b] > 1536u; big4 += m.nchunks[b] > 1024u; }
    double mx = 0, sum = 0; int nw = 0;                    // cost per workgroup: 1024 a block + its chunks
    for (int x = 0; x < 8; ++x) {
        double xs = 0, xm = 0; int xn = 0, xb = 0;
        for (int b = x; b < plan.grid; b += 8) {
            double cost = 0; int nbk = 0;
            for (int k = 0; k < plan.depth; ++k) { const int v = plan.assign[(size_t)b * plan.depth + k]; if (v >= 0) { cost += m.nchunks[(size_t)v]; ++nbk; } }
            if (nbk) { ++xn; xb += nbk; xs += cost; xm = std::max(xm, cost); ++nw; sum += cost + 1024.0 * nbk; mx = std::max(mx, cost + 1024.0 * nbk); }
        }
        fprintf(stderr, "RESIDENT plan XCD %d: %d workers, %d blocks, chunks per worker mean %.0f max %.0f\n", x, xn, xb, xn ? xs / xn : 0.0, xm);
    }
    fprintf(stderr, "RESIDENT plan: %u live blocks (max %u chunks, %d above 1024, %d above 1536), grid %d depth %d K %d nq %d lds %d, cost per workgroup mean %.0f max %.0f\n",
            (unsigned)m.order.size(), max_chunks, big4, big, plan.grid, plan.depth, c.form, res_nq(max_chunks), lds_buf, nw ? sum / nw : 0.0, mx);
}
// raw: every workgroup's word of d_up (workers leave 0x80000000 | figure behind); figures: the workers' figures, ascending
static void res_print_laggards(const Resident *R, const std::vector<uint32_t> &raw, const std::vector<uint32_t> &figures)
{
    if (FILE *df = fopen("gpurun_out/res_wg_stats.txt", "w")) {          // (developer: every workgroup's figure + its blocks' chunks / lines)
        for (size_t i = 0; i < raw.size(); ++i) {
            if (!(raw[i] & 0x80000000u)) continue;
            fprintf(df, "%zu %u", i, raw[i] & 0x7FFFFFFFu);
            for (int k = 0; k < R->depth; ++k) { const int v = R->plan_assign[i * R->depth + k]; if (v >= 0) fprintf(df, " %d:%u:%u", v, R->plan_hdr_chunks[(size_t)v], R->plan_lines[(size_t)v]); }
            fprintf(df, "\n");
        }
        fclose(df);
    }
    fprintf(stderr, "RESIDENT laggards (workgroup:streamed frames[chunks of its blocks]):");
    int shown = 0;
    const uint32_t cut = figures.size() > 16 ? figures[figures.size() - 16] : 0;
    for (size_t i = 0; i < raw.size() && shown < 24; ++i)
        if ((raw[i] & 0x80000000u) && (raw[i] & 0x7FFFFFFFu) >= cut) {
            fprintf(stderr, " %zu:%u[", i, raw[i] & 0x7FFFFFFFu);
            for (int k = 0; k < R->depth; ++k) { const int v = R->plan_assign[i * R->depth + k]; if (v >= 0) fprintf(stderr, "%u/%u ", R->plan_hdr_chunks[(size_t)v], R->plan_lines[(size_t)v]); }
            fprintf(stderr, "]");
            ++shown;
        }
    fprintf(stderr, "\n");
}

// at least `need` elements behind *p, of *cap allocated: if not, `alloc` new ones (what the old ones held was the last launch's)
template <typename T, typename N>
static int res_grow(bk_ctx *ctx, T **p, N *cap, size_t need, size_t alloc)
{
    if (*p && (size_t)*cap >= need) return BK_OK;
    (void)hipFree(*p); *p = nullptr; *cap = 0;
    BK_HIP(ctx, hipMalloc((void **)p, alloc * sizeof(T)));
    *cap = (N)alloc;
    return BK_OK;
}

static int res_grow_buffers(bk_ctx *ctx, Resident *R, const ResPlan &plan)
{
    const size_t nflags = (size_t)((plan.grid + 2048) / 2048 * 2048);      // (the collector reads the flags 2048 at a time)
    int cap_up = R->cap_wg, r = res_grow(ctx, &R->d_done, &R->cap_wg, (size_t)plan.grid, nflags);
    if (!r) r = res_grow(ctx, &R->d_up, &cap_up, (size_t)plan.grid, nflags);
    if (r) { R->cap_wg = 0; return r; }                  // (d_done and d_up: cap_wg words each, or to be allocated again)
    if ((r = res_grow(ctx, &R->d_assign, &R->cap_assign, plan.assign.size(), plan.assign.size()))) return r;
    return res_grow(ctx, &R->d_phase, &R->cap_phase, plan.phase.size(), std::max(plan.phase.size(), (size_t)R->cap_wg));
}

// the plan, the workgroups' flag words and an empty command ring, on the device before the kernel starts
static int res_upload_plan(bk_ctx *ctx, Resident *R, const ResPlan &plan)
{
    memset((void *)R->h, 0, sizeof(ResHost));
    // the flags: "done with everything" for the padding, the service workgroup and the sleepers; 0 for the workers
    std::vector<uint32_t> flags((size_t)R->cap_wg, 0xFFFFFFFFu);
    for (int b = 0; b < plan.grid; ++b) if (b != plan.service && plan.assign[(size_t)b * plan.depth] >= 0) flags[(size_t)b] = (uint32_t)plan.phase[(size_t)b];      // ("every frame of mine up to here": none yet)
    // (a worker the plan gave no block - possible with a frame stride, per-XCD rounding - would otherwise have to walk the tickets for nothing: it is "done with everything" and leaves)
    BK_HIP(ctx, hipMemcpyAsync(R->d_phase, plan.phase.data(), plan.phase.size() * sizeof(int), hipMemcpyHostToDevice, R->stream));
    BK_HIP(ctx, hipMemcpyAsync(R->d_done, flags.data(), flags.size() * sizeof(uint32_t), hipMemcpyHostToDevice, R->stream));
    BK_HIP(ctx, hipMemcpyAsync(R->d_assign, plan.assign.data(), plan.assign.size() * sizeof(int), hipMemcpyHostToDevice, R->stream));
    BK_HIP(ctx, hipMemsetAsync(R->d_ring, 0, ((size_t)BK_RES_MAX_COPIES * BK_RES_COPY_WORDS + 64) * sizeof(uint32_t), R->stream));
    BK_HIP(ctx, hipMemsetAsync(R->d_up, 0, (size_t)R->cap_wg * sizeof(uint32_t), R->stream));
    BK_HIP(ctx, hipStreamSynchronize(R->stream));                     // (the host vector above goes away)
    return BK_OK;
}

static ResArgs res_args(bk_ctx *ctx, const Resident *R, const CoopMap *cm, const ResChoice &c, int lds_buf)
{
    ResArgs a;
    a.hdr = cm->d_hdr; a.list = cm->d_list; a.idx = cm->d_idx; a.tint_t = ctx->d_tints; a.lmap = ctx->d_offsets;
    a.globe = ctx->d_globe; a.globe_stride = ctx->globe_stride(); a.globe_frames = ctx->nframes;
    a.W = ctx->W; a.rows = ctx->rows(); a.blocks_x = cm->blocks_x; a.nblocks = cm->blocks_x * cm->blocks_y; a.lds_buf = lds_buf;
    a.pal = R->d_pal; a.kflags = (ctx->apply_flags & BK_RF_KERNEL_MASK) | (R->direct ? BK_KF_DIRECT : 0);       // (the mask: see BkResidentFlag)
    a.rh = R->h; a.idle_ticks = (uint32_t)std::min(4.0e9, R->idle_ms * 1e5);
    a.ring = R->d_ring; a.wg_done = R->d_done; a.wg_up = R->d_up; a.nwg = c.plan.grid;
    a.exit_flag = R->d_ring + (size_t)BK_RES_MAX_COPIES * BK_RES_COPY_WORDS;
    a.assign = R->d_assign; a.depth = c.plan.depth; a.service = c.plan.service;
    a.ncopies = std::max(1, std::min(BK_RES_MAX_COPIES, (c.plan.grid + 15) / 16));
    // (direct submission: the HOST writes every copy, 32 bytes each through the BAR - 128 copies cost 4.4 us per submit; one to eight
    //  poll equally well (measured), four cost ~0.2 us)
    if (R->direct) a.ncopies = std::min(a.ncopies, 4);
    a.stride = c.stride; a.phase = R->d_phase;
    return a;
}

// every workgroup has to be ON the device: one that waits for a place would only start when the others leave.  The occupancy
// the API reports can be one more than the hardware admits (SGPR granules: MI355X_MICROARCH.md, "Residency"), so look.
// *resident = false: the kernel was sent away again, the next launch is to leave one place more per CU free
static int res_await_residency(bk_ctx *ctx, Resident *R, bool *resident)
{
    *resident = true;
    const uint64_t t0 = res_now_ns();
    while (R->h->up < (uint32_t)R->nwg - 1u && !R->h->exited) {
        if (res_now_ns() - t0 <= 50000000ull) continue;               // 50 ms
        const uint32_t up = R->h->up;
        if (int r = res_drain(ctx, R, true)) return r;
        if (R->shrink >= 6) return ctx->fail(BK_E_HIP, "resident apply: only %u of %d workgroups became resident", up, R->nwg);
        ++R->shrink;
        *resident = false;
        break;
    }
    return BK_OK;
}

// (re)launch the kernel for the context's current block map
// force_rg != 0: over blocks of that height (ensure_coopmap's force_rg) - a session growing its blocks
static int res_launch(bk_ctx *ctx, Resident *R, int shape_tries = 0, int force_rg = 0)
{
    // a session outlives resident_quiesce: after a bk_resize / bk_set_rows / failed bk_build in between there may be no lensmap (or
    // no rows) to compile a block map from - say so instead of launching on freed tables (bk_apply_device's answer to the same state)
    if (!ctx->lensmap_valid || !ctx->d_offsets || ctx->W <= 0 || ctx->rows() <= 0 || ctx->apply_variant == 0)
        return ctx->fail(BK_E_STATE, "resident apply: no lensmap for the current size / rows (bk_build or bk_set_lensmap first)");
    if (int r = ensure_coopmap(ctx, 1, R->rubix ? 1 : 0, force_rg)) return r;
    CoopMap *cm = ctx->coopmap;
    if (int r = coop_stats_wait(ctx, cm)) return r;
    ResMapHost m;
    if (int r = res_read_map(ctx, cm, &m)) return r;
    // the staging buffer holds the largest listed block of the map (the launch-per-frame kernel may run with a smaller one and
    // take such blocks in passes; here they would fall to the direct gather)
    int lds_buf = (int)std::min<uint32_t>(cm->stats[CS_MAX_CHUNKS], BK_COOP_MAX_CHUNKS + 1) * 16;
    lds_buf = std::max(1024, (lds_buf + 1023) & ~1023);
    const size_t staging = (size_t)lds_buf + (R->rubix ? BK_PAL_BYTES : 0);
    ResChoice c;
    if (int r = res_choose_form(ctx, R, cm, m, staging, shape_tries < 2 && !coop_forced_rg(ctx, force_rg) && cm->grown_rg != cm->rg, &c)) return r;
    if (c.verdict == ResChoice::NO_ROOM) return ctx->fail(BK_E_STATE, "resident apply: no room on the device for its workgroups (LDS %zu bytes each)", staging);
    if (c.verdict == ResChoice::GROW) {
        // the session's block map does not serve it at this block height: compile it twice as tall and launch over that; the map
        // remembers (`grown_rg`) that this height is a session's doing
        cm->valid = false;
        const int rc = res_launch(ctx, R, shape_tries + 1, cm->rg * 2);
        if (ctx->coopmap && ctx->coopmap->valid) ctx->coopmap->grown_rg = ctx->coopmap->rg;
        return rc;
    }
    if (g_debug.print_model) res_print_plan(m, c, cm->stats[CS_MAX_CHUNKS], lds_buf);
    if (int r = res_grow_buffers(ctx, R, c.plan)) return r;
    if (int r = res_upload_plan(ctx, R, c.plan)) return r;
    const ResArgs a = res_args(ctx, R, cm, c, lds_buf);
    R->plan_assign = c.plan.assign; R->plan_hdr_chunks = std::move(m.nchunks); R->plan_lines = std::move(m.lines);
    R->ncopies = a.ncopies; R->stride = c.stride; R->depth = c.plan.depth;
    R->nwg = c.plan.grid; R->K = c.form == 9 ? 3 : c.form == 10 ? 8 : c.form; R->NQ = res_nq(cm->stats[CS_MAX_CHUNKS]); R->rg = cm->rg; R->per_cu = c.places / ctx->num_cus;
    R->next_seq = 0;
    int places = 0;
    if (int r = res_variant_rg(ctx, R, cm->rg, a, c.shmem, c.form, R->NQ, true, &places)) return r;
    R->running = true;
    ++R->launches;
    bool resident = false;
    if (int r = res_await_residency(ctx, R, &resident)) return r;
    return resident ? BK_OK : res_launch(ctx, R, shape_tries, force_rg);
}

// the device copies of the command ring: fine-grained device memory the host can write through the BAR when the device has a large one
// (direct submission); else plain device memory fed by the relay wave
static hipError_t res_alloc_ring(bk_ctx *ctx, Resident *R)
{
    const size_t bytes = ((size_t)BK_RES_MAX_COPIES * BK_RES_COPY_WORDS + 64) * sizeof(uint32_t);
    hipDeviceProp_t prop;
    R->direct = false;
    if (!g_debug.no_direct_submit && hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.isLargeBar) {
        if (hipExtMallocWithFlags((void **)&R->d_ring, bytes, hipDeviceMallocFinegrained) == hipSuccess) { R->direct = true; return hipSuccess; }
        (void)hipGetLastError();
    }
    return hipMalloc((void **)&R->d_ring, bytes);
}

int resident_begin(bk_ctx *ctx, int rubix_on, double idle_ms)
{
    hw_queue_note();
    Resident *R = ctx->resident;
    if (!R) {
        R = ctx->resident = new Resident();
        if (hipHostMalloc((void **)&R->h, sizeof(ResHost), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
            res_alloc_ring(ctx, R) != hipSuccess ||
            hipMalloc((void **)&R->d_pal, BK_PAL_BYTES) != hipSuccess) {
            (void)hipGetLastError();
            resident_free(ctx);
            return ctx->fail(BK_E_NOMEM, "resident apply: cannot allocate its stream / command ring");
        }
    }
    if (R->running) { if (int r = res_drain(ctx, R, true)) return r; }
    if (!R->stream && hipStreamCreateWithFlags(&R->stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        return ctx->fail(BK_E_HIP, "resident apply: cannot create its stream");
    }
    R->shrink = 0;
    R->rubix = rubix_on != 0;
    // (fixed for the session, also across a transparent relaunch after somebody else's bk_apply replaced ctx->pal.d)
    if (R->rubix) BK_HIP(ctx, hipMemcpyAsync(R->d_pal, ctx->pal.d, BK_PAL_BYTES, hipMemcpyDeviceToDevice, ctx->stream));
    if (idle_ms > 0) R->idle_ms = idle_ms;
    R->base += R->next_seq;                    // tickets go on counting
    R->pending.clear();
    R->first_pending = R->base + 1;
    R->next_seq = 0;
    return res_launch(ctx, R);
}

// the kernel is gone (idle exit) with commands outstanding, or was never started again after one: start it and hand them over again
static int res_revive(bk_ctx *ctx, Resident *R)
{
    if (int r = res_drain(ctx, R, false)) return r;
    const uint32_t done = R->h->completed;                              // of the launch that ended
    // drop what that launch completed
    const uint64_t done_ticket = R->base + done;
    while (!R->pending.empty() && R->first_pending <= done_ticket) { R->pending.erase(R->pending.begin()); ++R->first_pending; }
    R->base = R->first_pending - 1;
    if (int r = res_launch(ctx, R)) return r;
    for (const Resident::Pending &p : R->pending) res_write_cmd(R, ++R->next_seq, BK_RES_FRAME, p.frame, p.pitch, p.dst);
    return BK_OK;
}

static int res_retire(Resident *R)
{
    const uint64_t done_ticket = R->base + R->h->completed;
    size_t n = 0;
    while (n < R->pending.size() && R->first_pending + n <= done_ticket) ++n;
    if (n) { R->pending.erase(R->pending.begin(), R->pending.begin() + (long)n); R->first_pending += n; }
    return BK_OK;
}

int resident_wait(bk_ctx *ctx, uint64_t ticket, double *gpu_us);

int resident_submit(bk_ctx *ctx, int frame, uint8_t *dst_first_owned_row, int dst_pitch, uint64_t *ticket)
{
    Resident *R = ctx->resident;
    if (!R) return ctx->fail(BK_E_STATE, "bk_apply_resident_submit without bk_apply_resident_begin");
    res_retire(R);
    if (R->pending.size() >= (size_t)BK_RES_RING / 2) {                 // keep half the ring free: wait for the oldest
        if (int r = resident_wait(ctx, R->first_pending, nullptr)) return r;
    }
    if (!R->running || R->h->exited) { if (int r = res_revive(ctx, R)) return r; }
    R->pending.push_back({(uint32_t)frame, dst_pitch, (uint64_t)(uintptr_t)dst_first_owned_row});
    res_write_cmd(R, ++R->next_seq, BK_RES_FRAME, (uint32_t)frame, dst_pitch, (uint64_t)(uintptr_t)dst_first_owned_row);
    if (ticket) *ticket = R->base + R->next_seq;
    return BK_OK;
}

int resident_wait(bk_ctx *ctx, uint64_t ticket, double *gpu_us)
{
    Resident *R = ctx->resident;
    if (!R) return ctx->fail(BK_E_STATE, "bk_apply_resident_wait without bk_apply_resident_begin");
    if (ticket > R->base + R->next_seq) return ctx->fail(BK_E_INVALID, "bk_apply_resident_wait: no such ticket");
    if (ticket >= R->lost_lo && ticket <= R->lost_hi)
        return ctx->fail(BK_E_STATE, "bk_apply_resident_wait: frame %llu was dropped unrendered (the session could not be resumed when it was ended)", (unsigned long long)ticket);
    int revived = 0;
    uint64_t t0 = res_now_ns();
    for (;;) {
        if (ticket <= R->base + R->h->completed) break;
        if (ticket < R->first_pending) break;                           // (retired earlier)
        if (R->h->exited || !R->running) {
            if (R->h->completed + R->base >= ticket) break;
            if (++revived > 3) return ctx->fail(BK_E_HIP, "resident apply: the kernel keeps leaving before frame %llu is done", (unsigned long long)ticket);
            if (int r = res_revive(ctx, R)) return r;
            t0 = res_now_ns();
            continue;
        }
        if (res_now_ns() - t0 > (uint64_t)(4.0 * R->idle_ms * 1e6) + 2000000000ull) {
            (void)res_drain(ctx, R, true);
            return ctx->fail(BK_E_HIP, "resident apply: frame %llu did not complete (completed %u of %u submitted, %u of %d workgroups up)",
                             (unsigned long long)ticket, R->h->completed, R->next_seq, R->h->up, R->nwg);
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (gpu_us && ticket > R->base) {
        const uint32_t slot = (uint32_t)((ticket - R->base - 1) % BK_RES_RING);
        *gpu_us = (double)(R->h->t_done[slot] - R->h->t_fwd[slot]) / 100.0;      // s_memrealtime: 100 MHz
    }
    res_retire(R);
    return BK_OK;
}

// leave: the kernel exits, the context is back to launches per call
int resident_stop(bk_ctx *ctx)
{
    Resident *R = ctx->resident;
    if (!R) return BK_OK;
    int rc = BK_OK;
    res_retire(R);
    if (!R->pending.empty()) {
        // "outstanding frames are finished first" - also when the kernel has left on its own (idle exit) with a command still
        // unforwarded: the wait brings it back for them.  Should that fail (no lensmap any more ...) the frames are LOST and a later
        // bk_apply_resident_wait on their tickets says so instead of reporting them complete
        rc = resident_wait(ctx, R->base + R->next_seq, nullptr);
        if (rc != BK_OK) {
            res_retire(R);
            if (!R->pending.empty()) { R->lost_lo = R->first_pending; R->lost_hi = R->base + R->next_seq; }
        }
    }
    if (R->running) {
        const int r2 = res_drain(ctx, R, true);
        if (rc == BK_OK) rc = r2;
        std::vector<uint32_t> st((size_t)R->nwg);
        if (R->nwg > 0 && hipMemcpy(st.data(), R->d_up, st.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess) {
            const std::vector<uint32_t> raw = st;              // (workers leave 0x80000000 | count behind; the service workgroup and the sleepers do not)
            {
                std::vector<uint32_t> w;
                for (uint32_t v : st) if (v & 0x80000000u) w.push_back(v & 0x7FFFFFFFu);
                if (w.empty()) w.push_back(0);
                st.swap(w);
            }
            const uint32_t mx0 = *std::max_element(st.begin(), st.end());
            R->streamed_argmax = 0;
            R->streamed_many = 0;
            for (size_t i = 0; i < raw.size(); ++i)
                if (raw[i] & 0x80000000u) {
                    if ((raw[i] & 0x7FFFFFFFu) == mx0) R->streamed_argmax = (int)i;
                    R->streamed_many += (raw[i] & 0x7FFFFFFFu) * 2 > mx0 ? 1 : 0;
                }
            std::sort(st.begin(), st.end());
            if (g_debug.print_model) res_print_laggards(R, raw, st);
            R->streamed_min = (int)st.front(); R->streamed_med = (int)st[st.size() / 2]; R->streamed_max = (int)st.back();
        }
    }
    R->base += R->next_seq;
    R->next_seq = 0;
    R->pending.clear();
    R->first_pending = R->base + 1;
    return rc;
}

void resident_free(bk_ctx *ctx)
{
    Resident *R = ctx->resident;
    if (!R) return;
    (void)resident_stop(ctx);
    if (R->stream) (void)hipStreamDestroy(R->stream);
    if (R->h) (void)hipHostFree((void *)R->h);
    (void)hipFree(R->d_ring); (void)hipFree(R->d_done); (void)hipFree(R->d_up); (void)hipFree(R->d_assign); (void)hipFree(R->d_pal); (void)hipFree(R->d_phase);
    delete R;
    ctx->resident = nullptr;
}

bool resident_running(bk_ctx *ctx) { Resident *R = ctx->resident; return R && R->running && !R->h->exited; }
// kernels of this context can run beside its resident kernel: a place per CU is reserved for them and the running form honoured it
bool resident_leaves_room(bk_ctx *ctx) { Resident *R = ctx->resident; return ctx->res_reserve > 0 && !(R && R->running && R->yielded); }

int resident_info(bk_ctx *ctx, int out[12])
{
    Resident *R = ctx->resident;
    for (int i = 0; i < 12; ++i) out[i] = 0;
    if (!R) return BK_OK;
    out[0] = R->running && !R->h->exited ? 1 : 0; out[1] = R->nwg; out[2] = R->K; out[3] = R->NQ; out[4] = 8 * R->rg; out[5] = R->per_cu;
    out[6] = (int)R->launches; out[7] = (int)R->pending.size();
    out[8] = R->streamed_min; out[9] = R->streamed_med; out[10] = R->streamed_max; out[11] = R->streamed_argmax * 10000 + R->streamed_many;
    return BK_OK;
}
