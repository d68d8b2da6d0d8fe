// resplan_check.cpp -- stand-alone check of the resident apply's planner (blinky_amd/csrc/bk_resident_plan.cpp): links that unit alone,
// no HIP, no Python.  Over a seeded sweep of synthetic block maps it holds every plan that reports "fits" to what the kernel and the
// collector rely on, the stride planner to refusing a plan with an empty stride group, and the form choice to its order of decisions.
// No plan is pinned: how blocks are balanced is free to change.  Prints what failed and exits non-zero; `make sanitize` builds it
// with AddressSanitizer + UndefinedBehaviorSanitizer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../blinky_amd/csrc/bk_resident_plan.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            if (++g_failed <= 40) {                              \
                fprintf(stderr, "resplan_check: FAILED %s: ", #cond); \
                fprintf(stderr, __VA_ARGS__);                    \
                fprintf(stderr, "\n");                           \
            }                                                    \
        }                                                        \
    } while (0)

struct Map {
    std::vector<uint32_t> nchunks, order;      // chunks per block; the live blocks in walk order
    std::vector<int> pos;                      // position in the walk of every block, -1 = not live
};

static uint32_t g_rng = 1;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (uint32_t)(((uint64_t)(g_rng >> 8) * n) >> 24); }

// nlive live blocks of 0 .. max_chunks chunks among a few dead ones, walked in an order of their own
static Map make_map(int nlive, uint32_t seed, uint32_t max_chunks = 1599)
{
    g_rng = seed * 2654435761u + 12345u;
    Map m;
    const int nblocks = nlive + nlive / 7 + 3;
    m.nchunks.resize((size_t)nblocks);
    for (uint32_t &c : m.nchunks) c = rnd(max_chunks + 1);
    std::vector<uint32_t> perm((size_t)nblocks);
    for (int i = 0; i < nblocks; ++i) perm[(size_t)i] = (uint32_t)i;
    for (int i = nblocks - 1; i > 0; --i) std::swap(perm[(size_t)i], perm[rnd((uint32_t)i + 1)]);
    m.order.assign(perm.begin(), perm.begin() + nlive);
    m.pos.assign((size_t)nblocks, -1);
    for (int i = 0; i < nlive; ++i) m.pos[m.order[(size_t)i]] = i;
    return m;
}

// what apply_resident_kernel and its collector take for granted of a plan
static void check_plan(const bk::ResPlan &P, const Map &m, int places, int stride, int cap, const std::string &what)
{
    const char *w = what.c_str();
    const int before = g_failed;
    CHECK(P.grid >= 9 && P.grid <= places, "%s: grid %d of %d places", w, P.grid, places);
    CHECK(P.service == P.grid - 1, "%s: service %d, grid %d", w, P.service, P.grid);
    CHECK(P.depth >= 1 && (cap == 0 || P.depth <= cap), "%s: depth %d, cap %d", w, P.depth, cap);
    CHECK(P.assign.size() == (size_t)P.grid * (size_t)P.depth, "%s: %zu assign entries for grid %d depth %d", w, P.assign.size(), P.grid, P.depth);
    CHECK(P.phase.size() == (size_t)P.grid, "%s: %zu phase entries for grid %d", w, P.phase.size(), P.grid);
    if (g_failed != before) return;
    std::vector<int> owners((size_t)stride * m.nchunks.size(), 0);
    int with_blocks = 0;
    for (int b = 0; b < P.grid; ++b) {
        const int *mine = &P.assign[(size_t)b * P.depth];
        const int ph = P.phase[(size_t)b];
        CHECK(ph >= 0 && ph < stride, "%s: workgroup %d has phase %d, stride %d", w, b, ph, stride);
        if (ph < 0 || ph >= stride) return;
        if (b == P.service) CHECK(mine[0] == -1, "%s: the service workgroup has a first entry %d", w, mine[0]);
        bool ended = false;
        int last = -1;
        for (int k = 0; k < P.depth; ++k) {
            const int v = mine[k];
            CHECK(v >= -1 || (v == -2 && k == 0), "%s: workgroup %d entry %d is %d", w, b, k, v);
            if (v < 0) { ended = true; continue; }
            CHECK(!ended, "%s: workgroup %d has block %d behind a hole", w, b, v);
            CHECK(b != P.service, "%s: the service workgroup has block %d", w, v);
            if ((size_t)v >= m.pos.size() || m.pos[(size_t)v] < 0) { CHECK(false, "%s: workgroup %d has block %d, which is not live", w, b, v); continue; }
            CHECK(m.pos[(size_t)v] > last, "%s: workgroup %d takes block %d out of walk order", w, b, v);
            last = m.pos[(size_t)v];
            ++owners[(size_t)ph * m.nchunks.size() + (size_t)v];
        }
        with_blocks += mine[0] >= 0;
    }
    CHECK(with_blocks <= P.workers, "%s: %d workgroups have blocks, %d workers", w, with_blocks, P.workers);
    for (int g = 0; g < stride; ++g)
        for (uint32_t blk : m.order) {
            const int n = owners[(size_t)g * m.nchunks.size() + blk];
            if (n != 1) { CHECK(n == 1, "%s: block %u has %d owners in stride group %d", w, blk, n, g); return; }
        }
}

static const int kLive[] = {0, 1, 2, 7, 8, 9, 24, 25, 63, 255, 510, 1530, 2040, 4050};
static const int kPlaces[] = {9, 10, 17, 64, 128, 256, 512, 1024, 2048};
static const int kCaps[] = {0, 1, 2, 3, 8};

static void sweep_plans(int *nplans, int *nfit)
{
    char what[160];
    for (int nlive : kLive)
        for (uint32_t seed = 1; seed <= 2; ++seed) {
            const Map m = make_map(nlive, seed * 100u + (uint32_t)nlive);
            for (int places : kPlaces) {
                for (int cap : kCaps)
                    for (int ncu : {256, 32, bk::RES_NO_SLEEPERS}) {
                        if (seed > 1 && ncu != 256) continue;
                        bk::ResPlan P;
                        bk::res_plan(m.nchunks, m.order, places, cap, (seed == 1 ? 4 : 6) * 256, ncu, &P);
                        snprintf(what, sizeof what, "res_plan(nlive %d seed %u, places %d, cap %d, ncu %d)", nlive, seed, places, cap, ncu);
                        ++*nplans;
                        // (seven sleepers and the service workgroup at the most: the rest are workers, and room under the cap is all it takes)
                        if (cap == 0 || (long long)(places - 8) * cap >= nlive) CHECK(P.fits, "%s refuses", what);
                        if (P.fits) { ++*nfit; check_plan(P, m, places, 1, cap, what); }
                    }
                for (int st = 2; st <= 8 && seed == 1; ++st)
                    for (int cap : {0, 1, 3}) {
                        bk::ResPlan P;
                        bk::res_plan_stride(m.nchunks, m.order, places, st, cap, &P);
                        snprintf(what, sizeof what, "res_plan_stride(nlive %d seed %u, places %d, stride %d, cap %d)", nlive, seed, places, st, cap);
                        ++*nplans;
                        // (every XCD has `st` workers or more and no cap: every group has workers, nothing to refuse)
                        if (cap == 0 && (places - 1) / 8 >= st) CHECK(P.fits, "%s refuses", what);
                        if (P.fits) { ++*nfit; check_plan(P, m, places, st, cap, what); }
                    }
            }
        }
}

// a stride group without a worker renders none of its frames, and the flag words of the others say it did
static void check_refusals()
{
    struct { int nlive, places, stride; } empty_group[] = {{1, 10, 8}, {7, 17, 3}};
    for (const auto &e : empty_group) {
        const Map m = make_map(e.nlive, 7);
        bk::ResPlan P;
        bk::res_plan_stride(m.nchunks, m.order, e.places, e.stride, 0, &P);
        CHECK(!P.fits, "res_plan_stride(nlive %d, places %d, stride %d) returns a plan with an empty stride group", e.nlive, e.places, e.stride);
    }
    // ... and one that has the room is taken: 255 blocks four times over on 2048 places, one block each
    const Map m = make_map(255, 7);
    bk::ResPlan P;
    bk::res_plan_stride(m.nchunks, m.order, 2048, 4, 1, &P);
    CHECK(P.fits, "res_plan_stride(nlive 255, places 2048, stride 4, cap 1) refuses");
    if (P.fits) check_plan(P, m, 2048, 4, 1, "res_plan_stride(255, 2048, 4, 1)");
}

// ---- the form choice: every rung of the ladder when, and only when, the rungs before it do not fit ----
struct Asked {
    std::vector<int> forms;
    std::vector<size_t> shmem;
};
static std::string list_of(const std::vector<int> &v)
{
    std::string s;
    for (int f : v) s += (s.empty() ? "" : " ") + std::to_string(f);
    return s;
}

namespace {
struct Rung {
    const char *name;
    int nlive;
    bk::ResChoiceIn in;
    int places;                          // of every form
    bk::ResChoice::Verdict verdict;
    int form;                            // (of a LAUNCH)
    std::vector<int> asked;              // the forms whose places were asked for, in this order
};
}  // namespace

static bk::ResChoiceIn choice_in(bool may_grow, int rg = 2, uint32_t max_chunks = 1000, size_t staging = 16384)
{
    bk::ResChoiceIn in;
    in.max_chunks = max_chunks; in.rg = rg; in.may_grow = may_grow; in.staging_bytes = staging;
    return in;
}

static void check_ladder()
{
    using C = bk::ResChoice;
    bk::ResChoiceIn no_tables = choice_in(false), tinted = choice_in(false), no_one = choice_in(false), no_stride = choice_in(false);
    no_tables.no_tables = true; tinted.tinted = true; no_one.no_one_block = true; no_stride.no_stride = true;
    // 64 places: 63 workers, eight on every XCD but the service workgroup's
    const std::vector<Rung> rungs = {
        {"a handful of blocks", 5, choice_in(true), 64, C::LAUNCH, 1, {1}},
        {"one block each, to the last worker", 63, choice_in(false), 64, C::LAUNCH, 1, {1}},
        {"2 x places", 120, choice_in(true), 64, C::LAUNCH, 2, {1, 2}},
        {"3 x places", 180, choice_in(true), 64, C::LAUNCH, 3, {1, 2, 3}},
        {"above 3 x places, may grow", 200, choice_in(true), 64, C::GROW, 0, {1, 2, 3}},
        {"above 3 x places, may grow but 32 rows already", 200, choice_in(true, 4), 64, C::LAUNCH, 4, {1, 2, 3, 4}},
        {"above 3 x places", 200, choice_in(false), 64, C::LAUNCH, 4, {1, 2, 3, 4}},
        {"above 4 x places", 300, choice_in(false), 64, C::LAUNCH, 6, {1, 2, 3, 4, 6}},
        {"above 6 x places", 450, choice_in(false), 64, C::LAUNCH, 8, {1, 2, 3, 4, 6, 8}},
        {"above 3 x places, no tables", 200, no_tables, 64, C::LAUNCH, 9, {1, 2, 3, 9}},
        {"above 3 x places, tinted", 200, tinted, 64, C::LAUNCH, 9, {1, 2, 3, 9}},
        {"above 8 x places", 600, choice_in(false), 64, C::LAUNCH, 10, {1, 2, 3, 4, 6, 8, 10, 9}},
        {"a handful of blocks, not the one-block form", 5, no_one, 64, C::LAUNCH, 2, {2}},
        {"blocks above 1024 chunks: six chunks per thread, no one-block form", 5, choice_in(false, 2, 1600), 64, C::LAUNCH, 2, {2}},
        // (1600 chunks: a table row is 6 KiB; 120000 bytes of staging leave room under the LDS ceiling for six rows, not for eight)
        {"the LDS ceiling", 600, choice_in(false, 2, 1600, 120000), 64, C::LAUNCH, 9, {2, 3, 4, 6, 9}},
        {"fewer than nine places", 5, choice_in(false), 8, C::NO_ROOM, 0, {1, 2, 3, 4, 6, 8, 10, 9}},
        // the second reason to grow: one block each just fits, no room for a second copy of the map
        {"just fits, may grow", 100, choice_in(true), 128, C::GROW, 1, {1}},
        {"just fits", 100, choice_in(false), 128, C::LAUNCH, 1, {1}},
        {"just fits, 64 blocks", 64, choice_in(true), 100, C::LAUNCH, 1, {1}},
        {"room for eight copies", 20, choice_in(true), 256, C::LAUNCH, 1, {1}},
        {"room for eight copies, no stride", 20, no_stride, 256, C::LAUNCH, 1, {1}},
    };
    for (const Rung &r : rungs) {
        const Map m = make_map(r.nlive, 11, std::min<uint32_t>(r.in.max_chunks, 1599));
        Asked asked;
        const C c = bk::res_choose(m.nchunks, m.order, r.in, [&](int form, size_t shmem) { asked.forms.push_back(form); asked.shmem.push_back(shmem); return r.places; });
        CHECK(c.verdict == r.verdict, "%s: verdict %d, expected %d", r.name, (int)c.verdict, (int)r.verdict);
        CHECK(asked.forms == r.asked, "%s: asked for the places of forms [%s], expected [%s]", r.name, list_of(asked.forms).c_str(), list_of(r.asked).c_str());
        if (c.verdict != C::LAUNCH || r.verdict != C::LAUNCH) continue;
        CHECK(c.form == r.form, "%s: form %d, expected %d", r.name, c.form, r.form);
        CHECK(c.places == r.places, "%s: places %d, expected %d", r.name, c.places, r.places);
        for (size_t i = 0; i < asked.forms.size(); ++i) {
            CHECK(asked.shmem[i] <= 160 * 1024 - 512, "%s: form %d asked for with %zu bytes of LDS", r.name, asked.forms[i], asked.shmem[i]);
            if (asked.forms[i] == c.form) CHECK(asked.shmem[i] == c.shmem, "%s: form %d asked for with %zu bytes of LDS, chosen with %zu", r.name, c.form, asked.shmem[i], c.shmem);
        }
        CHECK(c.shmem >= r.in.staging_bytes && (c.shmem > r.in.staging_bytes) == (c.form == 4 || c.form == 6 || c.form == 8 || c.form == 10), "%s: form %d with %zu bytes of LDS, %zu of them staging", r.name, c.form, c.shmem, r.in.staging_bytes);
        CHECK(c.stride >= 1 && c.stride <= 8 && (c.stride == 1 || (c.form <= 8 && !r.in.no_stride)), "%s: stride %d in form %d", r.name, c.stride, c.form);
        if (r.nlive == 20) CHECK((c.stride > 1) == !r.in.no_stride, "%s: stride %d", r.name, c.stride);
        check_plan(c.plan, m, r.places, c.stride, c.form <= 8 ? c.form : 0, r.name);
    }
    // a form that has fewer than nine places is as good as one that does not fit
    {
        const Map m = make_map(5, 11);
        const C c = bk::res_choose(m.nchunks, m.order, choice_in(false), [](int form, size_t) { return form == 1 ? 8 : 64; });
        CHECK(c.verdict == C::LAUNCH && c.form == 2, "form 1 has eight places: verdict %d form %d, expected form 2", (int)c.verdict, c.form);
    }
    // 9 versus 10: eight blocks resident (form 10) only where that is more than 0.15 of the map above what three (form 9) keep resident
    {
        const Map m = make_map(600, 11);
        int chose9 = 0, chose10 = 0, inside_margin = 0;
        for (int places10 = 16; places10 <= 64; ++places10) {
            bk::ResPlan p9, p10;
            bk::res_plan(m.nchunks, m.order, 64, 0, 4 * 256, 256, &p9);
            bk::res_plan(m.nchunks, m.order, places10, 0, 4 * 256, 256, &p10);
            const double r9 = std::min(1.0, 3.0 / p9.depth), r10 = std::min(1.0, 8.0 / p10.depth);
            bk::ResChoiceIn in = choice_in(false);
            in.ncu = 256;
            const C c = bk::res_choose(m.nchunks, m.order, in, [&](int form, size_t) { return form == 10 ? places10 : 64; });
            const int want = r10 > r9 + 0.15 ? 10 : 9;
            CHECK(c.verdict == C::LAUNCH && c.form == want, "9 or 10 with %d / 64 places (resident %.3f / %.3f): verdict %d form %d, expected form %d", places10, r10, r9, (int)c.verdict, c.form, want);
            if (c.verdict != C::LAUNCH) continue;
            CHECK(c.places == (c.form == 10 ? places10 : 64) && c.plan.depth == (c.form == 10 ? p10.depth : p9.depth), "9 or 10 with %d / 64 places: form %d with %d places, depth %d", places10, c.form, c.places, c.plan.depth);
            check_plan(c.plan, m, c.places, 1, 0, "9 or 10");
            chose9 += c.form == 9; chose10 += c.form == 10; inside_margin += r10 > r9 && r10 <= r9 + 0.15;
        }
        CHECK(chose9 > 0 && chose10 > 0 && inside_margin > 0, "9 or 10: %d times 9, %d times 10, %d inside the margin - the cases do not straddle it", chose9, chose10, inside_margin);
    }
}

int main()
{
    int nplans = 0, nfit = 0;
    sweep_plans(&nplans, &nfit);
    check_refusals();
    check_ladder();
    if (g_failed) { fprintf(stderr, "resplan_check: %d checks failed\n", g_failed); return 1; }
    printf("resplan_check ok: %d plans asked for, %d fit\n", nplans, nfit);
    return 0;
}
