// bk_resident_plan.h -- the resident apply's host decisions: which workgroup warps which blocks of the screen in which frame phase
// (the two planners), and which kernel form, grid and frame stride serve a block map (res_choose).  Plain values in, a plan out: no
// HIP, nothing of the context - the launcher (bk_apply_resident.inc) reads the map back, asks here, and launches what it is told.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace bk {
#pragma GCC visibility push(hidden)

// `grid` workgroups, the last one the service workgroup; assign[b * depth + k] is the k-th block of workgroup b in walk order, -1
// behind a worker's last block, -2 in the first place of a sleeper; phase[b] is b's stride group.  `fits`: every live block has an
// owner in every stride group and no worker more blocks than the cap asked for - a plan that does not fit has no `assign`.
struct ResPlan { int grid = 0, service = 0, depth = 1, workers = 0; bool fits = false; std::vector<int> assign, phase; };

constexpr int RES_NO_SLEEPERS = 0;      // for `ncu`: the device is shared between contexts, the service workgroup's CU gets workers too

// a block map is `nchunks` per block number and `order`, the live blocks in walk order.  depth_cap: most blocks a worker may hold
// (0 = as many as it takes); nq_chunks: what a block's register plan holds (cost only); res_plan_stride: the map dealt out
// `stride_groups` times over, to groups of workers that each take every stride_groups-th frame
void res_plan(const std::vector<uint32_t> &nchunks, const std::vector<uint32_t> &order, int places, int depth_cap, int nq_chunks, int ncu, ResPlan *P);
void res_plan_stride(const std::vector<uint32_t> &nchunks, const std::vector<uint32_t> &order, int places, int stride_groups, int depth_cap, ResPlan *P);

// chunks per thread of a block's register plan, by the most chunks of a listed block of the map
inline int res_nq(uint32_t max_chunks) { return max_chunks > 1024u ? 6 : 4; }

struct ResChoiceIn {                    // what the form choice goes by besides the map itself
    uint32_t max_chunks = 0;            // most chunks of a listed block (CS_MAX_CHUNKS)
    int rg = 4;                         // block height / 8
    bool tinted = false;                // rubix session: the register forms and the three-block tail only
    bool no_one_block = false, no_tables = false, no_stride = false;      // BK_RF_NO_ONE_BLOCK / BK_RF_NO_TABLES / BK_RF_NO_STRIDE
    bool may_grow = false;              // the caller may compile the map over blocks twice as tall and come again
    int ncu = RES_NO_SLEEPERS;          // CUs of the device, for the sleepers on the service workgroup's CU
    size_t staging_bytes = 0;           // LDS of a workgroup before any table: staging buffer (+ tint LUTs)
};
struct ResChoice {
    enum Verdict { LAUNCH, GROW, NO_ROOM } verdict = NO_ROOM;
    int form = 0;                       // 1 / 2 / 3 blocks in registers, 4 / 6 / 8 in an LDS table, 9 / 10: three / eight resident and a per-frame tail
    int places = 0, stride = 1;
    size_t shmem = 0;                   // LDS of a workgroup in that form
    ResPlan plan;
};
// places_of: workgroups of `form` with `shmem_bytes` of LDS each that the device holds at once (0: none, or it could not be asked)
using ResPlacesOf = std::function<int(int form, size_t shmem_bytes)>;
ResChoice res_choose(const std::vector<uint32_t> &nchunks, const std::vector<uint32_t> &order, const ResChoiceIn &in, const ResPlacesOf &places_of);

#pragma GCC visibility pop
}  // namespace bk
