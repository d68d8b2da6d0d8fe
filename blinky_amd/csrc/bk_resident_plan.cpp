// bk_resident_plan.cpp -- the resident apply's planners and its choice of kernel form (bk_resident_plan.h).  Stands alone: the standard
// library only, linked into tests/host/resplan_check.cpp without the rest of the library.
#include "bk_resident_plan.h"

#include <algorithm>

namespace bk {

// Who does what.  The grid is `places` workgroups (all of them resident at once); the last one is the service workgroup, and the
// seven that share its CU - the hardware deals an XCD's workgroups round the XCD's 32 CUs: grid positions service - ncu m - sleep,
// when the grid is large enough for it to matter.  A worker with grid position b runs on XCD b % 8 (observed dispatch order,
// MI355X_MICROARCH.md; only locality hangs on it).
struct ResRoles {
    int grid = 0;
    std::vector<int> sleepers;          // grid positions
    std::vector<int> wpos;              // grid position of worker w; the workers are numbered in grid order
    std::vector<int> wx[8];             // the workers of every XCD
};

// (the workgroups b and b + ncu share a CU: an XCD's workgroups go round its CUs)
static int res_sleepers(int grid, int ncu) { return ncu > 0 && grid / 4 >= ncu ? std::min(7, (grid - 1) / ncu) : 0; }

// the roles of the largest grid <= places that has no more than `want` workers (0: no such wish), nine workgroups at the least
static ResRoles res_roles(int places, int want, int ncu)
{
    ResRoles ro;
    ro.grid = places;
    // (a workgroup less is a worker less or - where it takes a sleeper along - none: the walk down cannot step over `want`)
    while (want > 0 && ro.grid > 9 && ro.grid - 1 - res_sleepers(ro.grid, ncu) > want) --ro.grid;
    std::vector<char> sleeps((size_t)ro.grid, 0);
    for (int m = 1; m <= res_sleepers(ro.grid, ncu); ++m) sleeps[(size_t)(ro.grid - 1 - ncu * m)] = 1;
    for (int b = 0; b < ro.grid - 1; ++b) {
        if (sleeps[(size_t)b]) { ro.sleepers.push_back(b); continue; }
        ro.wx[b & 7].push_back((int)ro.wpos.size());
        ro.wpos.push_back(b);
    }
    return ro;
}

// mine[w]: positions in `order` of worker w's blocks
static void res_assign(const ResRoles &ro, const std::vector<uint32_t> &order, std::vector<std::vector<int>> &mine, int depth, ResPlan *P)
{
    P->depth = depth;
    P->assign.assign((size_t)ro.grid * depth, -1);
    for (int b : ro.sleepers) P->assign[(size_t)b * depth] = -2;
    for (size_t w = 0; w < mine.size(); ++w) {
        // a worker takes its blocks in walk order, so that at any moment the workers of an XCD are still on neighbouring pieces of the screen
        std::sort(mine[w].begin(), mine[w].end());
        for (size_t k = 0; k < mine[w].size(); ++k) P->assign[(size_t)ro.wpos[w] * depth + k] = (int)order[(size_t)mine[w][k]];
    }
}

// A worker takes blocks of "its" XCD's share of the live blocks in walk order, the shares cut so that their cost is proportional to
// the XCD's workers; inside a share the dearest block goes to the worker that has the least so far - the frame is as long as its
// slowest workgroup, and whole-globe lenses have blocks of 300 and of 1500 chunks.  cost of a block = 256 + its chunks (measured: a
// workgroup's frame time goes with the chunks it stages) + 1200 if it overflows the register plan.
void res_plan(const std::vector<uint32_t> &nchunks, const std::vector<uint32_t> &order, int places, int depth_cap, int nq_chunks, int ncu, ResPlan *P)
{
    const int nlive = (int)order.size();
    // one block each when the map allows it: no more workgroups than blocks (+ the service CU's)
    const ResRoles ro = res_roles(places, nlive, ncu);
    const int workers = (int)ro.wpos.size();
    auto cost_of = [&](uint32_t blk) { return 256.0 + (double)nchunks[blk] + (nchunks[blk] > (uint32_t)nq_chunks ? 1200.0 : 0.0); };
    // Which XCD takes which blocks.  The walk is cut into SEGMENTS of 24 consecutive live blocks (the walk goes down patches of 8
    // block rows column by column: a segment is a compact 3 x 8 piece of the screen, most of a block's neighbours - the blocks it
    // shares globe lines with - are in its own segment), and the segments are dealt to the XCDs dearest first, each to the XCD
    // that has the least cost per worker so far and room left (a worker holds at most depth_cap blocks).  Contiguous eighths of
    // the walk - one stretch per XCD, as the launch-per-frame kernel's bands - cannot be balanced by cost AND by count at once:
    // 4K hammer in three blocks per worker left 2360 chunks per worker on the XCDs that own the cube's corners and 1306 on the
    // ones in between, and the frame is as long as its slowest workgroup.
    std::vector<std::vector<int>> xb(8);                        // per XCD: positions in `order`
    {
        const int SEG = 24;
        struct Seg { int lo, hi; double cost; };
        std::vector<Seg> segs;
        for (int l = 0; l < nlive; l += SEG) {
            Seg sg = {l, std::min(nlive, l + SEG), 0.0};
            for (int i = sg.lo; i < sg.hi; ++i) sg.cost += cost_of(order[(size_t)i]);
            segs.push_back(sg);
        }
        std::sort(segs.begin(), segs.end(), [](const Seg &p, const Seg &q) { return p.cost > q.cost || (p.cost == q.cost && p.lo < q.lo); });
        std::vector<double> xcost(8, 0.0);
        for (const Seg &sg : segs) {
            int l = sg.lo;
            while (l < sg.hi) {
                int best = -1;
                for (int x = 0; x < 8; ++x) {
                    const int nw = (int)ro.wx[x].size();
                    if (nw == 0) continue;
                    const int room = depth_cap > 0 ? nw * depth_cap - (int)xb[(size_t)x].size() : nlive;
                    if (room <= 0) continue;
                    if (best < 0 || xcost[(size_t)x] / nw < xcost[(size_t)best] / (double)ro.wx[best].size()) best = x;
                }
                if (best < 0) break;                            // (does not fit under the cap: the caller tries the next form)
                const int nw = (int)ro.wx[best].size();
                const int room = depth_cap > 0 ? nw * depth_cap - (int)xb[(size_t)best].size() : nlive;
                const int take = std::min(room, sg.hi - l);     // (a segment that does not fit whole is split)
                for (int i = 0; i < take; ++i) { xb[(size_t)best].push_back(l + i); xcost[(size_t)best] += cost_of(order[(size_t)(l + i)]); }
                l += take;
            }
            if (l < sg.hi) break;
        }
    }
    int placed = 0, depth = 1;
    for (int x = 0; x < 8; ++x) {
        const int nb = (int)xb[(size_t)x].size(), nw = (int)ro.wx[x].size();
        placed += nb;
        if (nw > 0) depth = std::max(depth, (nb + nw - 1) / nw);
    }
    P->grid = ro.grid; P->service = ro.grid - 1; P->depth = depth; P->workers = workers;
    P->phase.assign((size_t)ro.grid, 0);
    P->assign.clear();
    P->fits = placed == nlive;
    if (!P->fits) return;
    std::vector<std::vector<int>> mine((size_t)workers);
    for (int x = 0; x < 8; ++x) {
        const std::vector<int> &w = ro.wx[x];
        const int nw = (int)w.size();
        if (nw == 0) continue;
        // the dearest block first, each to the worker that has the least so far and still a place free
        std::vector<double> have((size_t)nw, 0.0);
        std::vector<int> cnt((size_t)nw, 0), bidx = xb[(size_t)x];
        std::sort(bidx.begin(), bidx.end(), [&](int p, int q) { const double cp = cost_of(order[(size_t)p]), cq = cost_of(order[(size_t)q]); return cp > cq || (cp == cq && p < q); });
        // (a heap of workers by load: 3000 blocks x 128 workers needs no better than a scan)
        for (int l : bidx) {
            int best = -1;
            for (int i = 0; i < nw; ++i)
                if (cnt[(size_t)i] < depth && (best < 0 || have[(size_t)i] < have[(size_t)best])) best = i;
            if (best < 0) break;
            mine[(size_t)w[(size_t)best]].push_back(l);
            ++cnt[(size_t)best];
            have[(size_t)best] += cost_of(order[(size_t)l]);
        }
    }
    res_assign(ro, order, mine, depth, P);
}

// Who does what when the map is dealt out to several STRIDE GROUPS (r5).  A workgroup's frame time goes with the NUMBER of its blocks first
// and with their bytes second (profiles/r05_resident_apply.txt), so every worker of a group gets the same number of blocks (+- 1) and,
// within that, the same cost.  XCD x (grid position % 8) takes a contiguous stretch of the walk - neighbouring
// blocks share globe lines, and an XCD's L2 is where they meet - whose length is proportional to its workers; inside the stretch
// the dearest block goes to the worker with the least cost among those with the fewest blocks.  A strided grid has no sleepers.
void res_plan_stride(const std::vector<uint32_t> &nchunks, const std::vector<uint32_t> &order, int places, int stride_groups, int depth_cap, ResPlan *P)
{
    const int nlive = (int)order.size();
    // no more workers than block copies - plus a few: the groups take an XCD's workers in turn, so their sizes differ by up to one
    // worker per XCD, and every group needs a worker per block
    const ResRoles ro = res_roles(places, nlive > 0 ? nlive * stride_groups + (stride_groups > 1 ? 8 * stride_groups : 0) : 0, RES_NO_SLEEPERS);
    const int workers = (int)ro.wpos.size();
    P->grid = ro.grid; P->service = ro.grid - 1; P->depth = 1; P->workers = workers;
    P->phase.assign((size_t)ro.grid, 0);
    P->assign.clear();
    P->fits = true;
    std::vector<std::vector<int>> mine((size_t)workers);
    for (int g = 0; g < stride_groups; ++g) {
        // this group's workers, by XCD: every XCD's workers go to the groups in turn, so that every group - every frame - is spread over
        // all eight XCDs ("worker w to group w % stride" would put a whole group on ONE XCD when the stride is 8: consecutive grid
        // positions are the eight XCDs)
        std::vector<int> wx[8];
        int ngw = 0;
        for (int x = 0; x < 8; ++x)
            for (size_t i = (size_t)g; i < ro.wx[x].size(); i += (size_t)stride_groups) { wx[x].push_back(ro.wx[x][i]); P->phase[(size_t)ro.wpos[(size_t)ro.wx[x][i]]] = g; ++ngw; }
        // (a small grid: fewer than `stride_groups` workers on every XCD leave the later groups without any, and their frames unrendered)
        if (ngw == 0) { P->fits = P->fits && nlive == 0; continue; }
        // stretches of the walk by worker count (largest remainder keeps the per-worker counts within one of each other)
        int lo = 0, wseen = 0;
        for (int x = 0; x < 8; ++x) {
            const int nw = (int)wx[x].size();
            wseen += nw;
            const int hi = (int)((long long)nlive * wseen / ngw);
            if (nw > 0) {
                std::vector<int> idx;
                for (int l = lo; l < hi; ++l) idx.push_back(l);
                std::sort(idx.begin(), idx.end(), [&](int p, int q) { const uint32_t cp = nchunks[order[(size_t)p]], cq = nchunks[order[(size_t)q]]; return cp > cq || (cp == cq && p < q); });
                std::vector<double> have((size_t)nw, 0.0);
                std::vector<int> cntw((size_t)nw, 0);
                for (int l : idx) {
                    int best = 0;
                    for (int i = 1; i < nw; ++i)
                        if (cntw[(size_t)i] < cntw[(size_t)best] || (cntw[(size_t)i] == cntw[(size_t)best] && have[(size_t)i] < have[(size_t)best])) best = i;
                    mine[(size_t)wx[x][(size_t)best]].push_back(l);
                    have[(size_t)best] += 256.0 + nchunks[order[(size_t)l]];
                    ++cntw[(size_t)best];
                }
            }
            lo = hi;
        }
    }
    for (auto &m : mine) P->depth = std::max(P->depth, (int)m.size());
    P->fits = P->fits && (depth_cap == 0 || P->depth <= depth_cap);
    if (P->fits) res_assign(ro, order, mine, P->depth, P);
}

// The smallest form whose grid holds every block of the map on the chip: one, two or three blocks per workgroup with their chunk
// offsets in registers; if the map needs more, blocks twice as tall first (a workgroup's frame time goes with the NUMBER of its
// blocks - one trip to memory each, measured 2.5 us - so the same screen in taller blocks is less work: 4K mercator at 128 x 16 is
// 4050 live blocks, at 128 x 32 half that); then (r5) four, six or eight blocks per workgroup with the offsets in an LDS table;
// and only a map that exceeds that too (8K: its chunk offsets alone are the size of the chip's LDS) keeps eight (or three) blocks
// per workgroup resident and fetches the rest of its block map per frame, as a launch would.
ResChoice res_choose(const std::vector<uint32_t> &nchunks, const std::vector<uint32_t> &order, const ResChoiceIn &in, const ResPlacesOf &places_of)
{
    ResChoice c;
    const int nq = res_nq(in.max_chunks);
    const uint32_t tab_row = std::min<uint32_t>((in.max_chunks + 255u) & ~255u, (uint32_t)nq * 256u) * 4u;      // bytes of table per block, worst case
    auto form_shmem = [&](int form) -> size_t { return in.staging_bytes + (form == 4 || form == 6 || form == 8 ? (size_t)form * tab_row : form == 10 ? 8 * (size_t)tab_row : 0); };
    const bool tables = !in.no_tables && !in.tinted;        // (rubix - a debugging view - has the register forms and the tail, not the table forms)
    // (r6: ... and not from a map that a session's growth produced already - the caller's `grown_rg`: the next session of the same lensmap used
    //  to find session 1's 128 x 16 map, grow it once more and take a form session 1 had not even looked at: 4K gumby 14.9 us per frame in the
    //  first session, 35.5 in every later one, 256 workgroups of eight 128 x 32 blocks each)
    const bool may_grow = in.rg < 4 && in.may_grow;
    // `form` with at most depth_cap blocks per workgroup (0: any number): its places and its plan, if it has room for the map
    auto try_form = [&](int form, int depth_cap, int *places, ResPlan *plan) -> bool {
        if (form_shmem(form) > 160 * 1024 - 512) return false;
        *places = places_of(form, form_shmem(form));
        if (*places < 9) return false;
        res_plan(nchunks, order, *places, depth_cap, (form == 1 ? 4 : nq) * 256, in.ncu, plan);
        return plan->fits;
    };
    auto first_of = [&](std::initializer_list<int> forms) -> bool {
        for (int form : forms) {
            if (form == 1 && (nq > 4 || in.no_one_block)) continue;
            if (try_form(form, form, &c.places, &c.plan)) { c.form = form; return true; }
        }
        return false;
    };
    bool ok = first_of({1, 2, 3});
    if (!ok && may_grow) { c.verdict = ResChoice::GROW; return c; }
    if (!ok && tables) ok = first_of({4, 6, 8});
    if (!ok) {
        // does not fit the chip: the rest is fetched per frame - with eight blocks resident (table) or with three (registers), whichever
        // leaves less of the map to fetch
        ResPlan p10;
        int places10 = 0;
        const bool ok10 = tables && try_form(10, 0, &places10, &p10), ok9 = try_form(9, 0, &c.places, &c.plan);
        const double resident9 = ok9 ? std::min(1.0, 3.0 / std::max(1, c.plan.depth)) : -1.0, resident10 = ok10 ? std::min(1.0, 8.0 / std::max(1, p10.depth)) : -1.0;
        c.form = 9;
        ok = ok9;
        if (resident10 > resident9 + 0.15) { c.form = 10; c.plan = p10; c.places = places10; ok = true; }
    }
    if (!ok) return c;
    // (r5) FRAME STRIDE: the plan uses a fraction of the places the form has (a 270-row stripe of a 4K frame is 255 blocks of 128 x 32 on
    // 2048 places; 1080p is 510) - deal the map out `stride` times over, group p taking the frames p + 1, p + 1 + stride, ...  One frame
    // at a time is not faster for it (a frame is still one trip per block), pipelined submissions are: `stride` frames side by side.
    // A stride whose plan does not fit - a worker with more than `form` blocks, a group without workers - leaves it to the next smaller one.
    const int K = c.form;
    if (K >= 1 && K <= 8 && !in.no_stride && c.plan.grid > 9) {
        const int per_group = ((int)order.size() + K - 1) / K;              // workers one copy of the map needs at K blocks each
        const int room = (c.places - 1) / std::max(1, per_group);
        for (int st = std::min(8, room); st >= 2; --st) {
            ResPlan p2;
            res_plan_stride(nchunks, order, c.places, st, K, &p2);
            if (p2.fits) { c.plan = p2; c.stride = st; break; }
        }
    }
    // ... and a map of one block per workgroup that just fits (1080p hammer at 128 x 8: 1530 blocks on 2048 places) has no room for a
    // second copy: blocks twice as tall are half as many, a trip to memory is hardly longer for them, and the stride doubles - 3.6 us per
    // pipelined frame at 128 x 8, 1.35 at 128 x 32 with five frames side by side (stereographic, measured)
    const bool just_fits = c.stride == 1 && K == 1 && (int)order.size() * 2 > c.places && (int)order.size() > 64;
    c.verdict = just_fits && may_grow ? ResChoice::GROW : ResChoice::LAUNCH;
    c.shmem = form_shmem(K);
    return c;
}

}  // namespace bk
