// host_mirror_test.cpp — exercises include/vecgo_hip.hpp (the C++ mirror of the reference's Go
// interfaces) the way the reference's own tests exercise the Go ones:
//   internal/quantization/pq_test.go:10-140, rabitq_test.go:10-97, internal/kmeans/kmeans_test.go:12-93,
//   distance/distance_test.go, internal/segment/flat/pq_test.go:17-93.
// The flat search is checked bit-for-bit against the CPU oracle (test infrastructure).
// The host-only plan of the HNSW builders (vg_build_plan.hpp) is checked first, against the oracle's schedule and
// layout: that part needs no device.
// Exit code 0 = all checks passed; 77 = no gfx950 device (the mirror refused to run: there is no
// CPU fallback) and the host-only checks passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../vecgo_amd/csrc/vg_build_plan.hpp"
#include "../../vecgo_amd/csrc/vg_int4_plan.hpp"
#include "../../vecgo_amd/csrc/vg_scan_slices.hpp"
#include "../../vecgo_amd/csrc/vg_walk_chunk.hpp"
#include "vecgo_hip.hpp"
#include "vg_oracle.h"

using namespace vecgo;
using quantization::ProductQuantizer;
using quantization::RaBitQuantizer;

static int g_fail = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                        \
        }                                                                    \
    } while (0)

template <typename F>
static int32_t status_of(F f)
{
    try {
        f();
    } catch (const Error &e) {
        return e.status();
    }
    return VG_OK;
}

static std::vector<std::vector<float>> unit_vectors(std::mt19937 &rng, int n, int dim)
{
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> out(n, std::vector<float>(dim));
    for (auto &v : out) {
        double s = 0;
        for (auto &x : v) {
            x = nd(rng);
            s += double(x) * x;
        }
        const float inv = float(1.0 / std::sqrt(s));
        for (auto &x : v) x *= inv;
    }
    return out;
}

// what a host allocates per query for the graph searches' counters (the struct grew from 4 to 5 fields)
static_assert(sizeof(vg_search_stats) == 5 * sizeof(int64_t), "vg_search_stats is five int64: bump VG_ABI_VERSION with it");

// the queries of one launch of a graph walk (WalkChunks, vg_search.hpp): a cap below one query's scratch still walks one
// query, a cap above the whole batch's takes the batch, in between the exact quotient
static_assert(vg::walk_chunk(int64_t(1) << 30, (int64_t(1) << 30) + 1, 8192) == 1, "a query that does not fit walks alone");
static_assert(vg::walk_chunk(int64_t(1) << 30, 650000, 8192) == 1651, "1 GiB of 650 000-byte queries: floor(2^30 / 650 000)");
static_assert(vg::walk_chunk(int64_t(16) << 30, 650000, 8192) == 8192, "room for more than the batch: the batch");
static_assert(vg::walk_chunk(int64_t(1) << 30, 131072, 8192) == 8192 && vg::walk_chunk(int64_t(1) << 30, 131073, 8192) == 8191,
              "the quotient is exact at the boundary");
static_assert(vg::walk_chunk(int64_t(1) << 30, 0, 5) == 5 && vg::walk_chunk(0, 100, 5) == 1, "no scratch per query; no room at all");

// the slices of a whole-segment code scan (vg_scan_slices.hpp): SQ8 and RaBitQ ask for 4 workgroups per CU over the
// segment's tiles, the PQ ADC scan for 1 over its 8-wave groups of tiles; a multiple of 8, never more than the tiles allow
static_assert(vg::scan_slices(1, 15625, 256, 4) == 1024, "one query, 1M rows: 4 workgroups on each of 256 CUs");
static_assert(vg::scan_slices(3, 15625, 256, 4) == 344, "ceil(1024 / 3) = 342, up to a multiple of 8");
static_assert(vg::scan_slices(256, 15625, 256, 4) == 8, "enough units per slice: one slice per XCD");
static_assert(vg::scan_slices(1, 100, 256, 4) == 96, "100 tiles: the multiple of 8 below");
static_assert(vg::scan_slices(1, 5, 256, 4) == 8, "fewer tiles than XCDs: still 8");
static_assert(vg::scan_slices(1, 1954, 256, 1) == 256, "ADC, 1M rows in groups of 8 waves: one workgroup per CU");
static_assert(vg::scan_slices(1024, 1954, 256, 1) == 8, "ADC, more queries than CUs");
// the sizes of tests/test_gpu_scan_trips.py on 256 CUs (tests/test_scan_shapes_cpu.py pins tests/scan_shapes.py to the same lines)
static_assert(vg::scan_slices(1, 4688, 256, 4) == 1024, "300 001 rows: 4688 tiles over 4096 dealt waves, trips 2 / 1 (SQ8 4 waves, RaBitQ)");
static_assert(vg::scan_slices(1, 586, 256, 1) == 256, "300 001 rows in groups of 8 tiles: 2048 dealt waves, trips 3 / 2 (ADC)");
static_assert(vg::scan_slices(1, 9376, 256, 4) == 1024, "600 001 rows: 9376 tiles, trips 3 / 2 at 4 waves (RaBitQ ring)");
static_assert(9376 >= 8 * vg::scan_slices(1, 9376, 256, 4) && 4688 < 8 * vg::scan_slices(1, 4688, 256, 4),
              "600 001 rows reach the SQ8 8-wave workgroup (trips 2 / 1), 300 001 do not");
static_assert(vg::scan_slices(65, 313, 256, 4) == 16, "20 000 rows, 1030 RaBitQ queries in blocks of 16");
static_assert(vg::scan_slices(150, 313, 256, 4) == 8, "20 000 rows, 600 SQ8 queries in groups of 4");

// the kernel and launch shape of a one-query INT4 distance scan (vg_int4_plan.hpp): arguments (dim, codes 16-byte aligned, rows,
// CUs, test hook VG_INT4_SMALL_GRID) -> kernel, waves per workgroup, workgroups, dynamic LDS bytes.  tests/test_scan_shapes_cpu.py
// pins tests/scan_shapes.py to the same lines.  These are the launches vg_int4_l2_distance_batch made before the rule moved
// into the header: dim % 256 == 0 up to 1024 the table scan on min(ceil(tiles / waves), CUs) workgroups, other dim % 64 == 0
// the pair-table scan on ceil(tiles / 4), everything else a lane per row in workgroups of 256.
constexpr bool i4_is(vg::Int4ScanPlan p, int32_t kernel, int32_t waves, int64_t blocks, int64_t lds)
{
    return p.kernel == kernel && p.waves == waves && p.blocks == blocks && p.lds == lds;
}
#define I4_PLAN(DIM, ALIGNED, N, CUS, HOOK, KERNEL, WAVES, BLOCKS, LDS) \
    static_assert(i4_is(vg::int4_scan_plan(DIM, ALIGNED, N, CUS, HOOK), vg::KERNEL, WAVES, BLOCKS, LDS), #DIM " " #ALIGNED " " #N " " #CUS " " #HOOK)
// a tail piece of 32, 64, 96 bytes alone and behind whole pieces; unaligned codes: a lane per row whatever the dimension
I4_PLAN(64, true, 1000000, 256, false, kI4PairTail, 4, 3907, 0);
I4_PLAN(64, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(128, true, 1000000, 256, false, kI4PairTail, 4, 3907, 0);
I4_PLAN(128, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(192, true, 1000000, 256, false, kI4PairTail, 4, 3907, 0);
I4_PLAN(192, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(320, true, 1000000, 256, false, kI4PairTail, 4, 3907, 0);
I4_PLAN(320, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(1088, true, 1000000, 256, false, kI4PairTail, 4, 3907, 0);
I4_PLAN(1088, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
// whole 128-byte pieces above the table scan's 1024 dimensions
I4_PLAN(1280, true, 1000000, 256, false, kI4Pair128, 4, 3907, 0);
I4_PLAN(1280, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(1536, true, 1000000, 256, false, kI4Pair128, 4, 3907, 0);
I4_PLAN(1536, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(3072, true, 1000000, 256, false, kI4Pair128, 4, 3907, 0);
I4_PLAN(3072, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(1536, true, 5, 256, true, kI4Pair128, 4, 1, 0);        // (the hook touches the table scan alone)
I4_PLAN(1536, true, 833, 256, false, kI4Pair128, 4, 4, 0);
// dim % 64 != 0
I4_PLAN(2056, true, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(2056, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(2056, true, 130, 256, true, kI4Row, 4, 1, 0);
I4_PLAN(95, true, 130, 256, false, kI4Row, 4, 1, 0);
// the table scan: 12 waves beside the table, 10 at dim 1024; workgroups capped by the CUs, by the hook at 2, and never
// more than the tiles ask for (3000 rows: 47 tiles; 65 rows: 2)
I4_PLAN(256, true, 1000000, 256, false, kI4Tab, 12, 256, 126976);
I4_PLAN(256, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(768, true, 1000000, 256, false, kI4Tab, 12, 256, 159744);
I4_PLAN(768, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(1024, true, 1000000, 256, false, kI4Tab, 10, 256, 157696);
I4_PLAN(1024, false, 1000000, 256, false, kI4Row, 4, 3907, 0);
I4_PLAN(256, true, 1000000, 304, false, kI4Tab, 12, 304, 126976);
I4_PLAN(256, true, 1000000, 256, true, kI4Tab, 12, 2, 126976);
I4_PLAN(256, true, 3000, 256, false, kI4Tab, 12, 4, 126976);
I4_PLAN(256, true, 3000, 256, true, kI4Tab, 12, 2, 126976);
I4_PLAN(256, true, 65, 256, true, kI4Tab, 12, 1, 126976);
I4_PLAN(256, true, 1, 0, false, kI4Tab, 12, 1, 126976);
I4_PLAN(512, true, 1000000, 304, false, kI4Tab, 12, 304, 143360);
I4_PLAN(512, true, 1000000, 256, true, kI4Tab, 12, 2, 143360);
I4_PLAN(512, true, 3000, 256, false, kI4Tab, 12, 4, 143360);
I4_PLAN(512, true, 3000, 256, true, kI4Tab, 12, 2, 143360);
I4_PLAN(512, true, 65, 256, true, kI4Tab, 12, 1, 143360);
I4_PLAN(512, true, 1, 0, false, kI4Tab, 12, 1, 143360);
I4_PLAN(768, true, 1000000, 304, false, kI4Tab, 12, 304, 159744);
I4_PLAN(768, true, 1000000, 256, true, kI4Tab, 12, 2, 159744);
I4_PLAN(768, true, 3000, 256, false, kI4Tab, 12, 4, 159744);
I4_PLAN(768, true, 3000, 256, true, kI4Tab, 12, 2, 159744);
I4_PLAN(768, true, 65, 256, true, kI4Tab, 12, 1, 159744);
I4_PLAN(768, true, 1, 0, false, kI4Tab, 12, 1, 159744);
I4_PLAN(1024, true, 1000000, 304, false, kI4Tab, 10, 304, 157696);
I4_PLAN(1024, true, 1000000, 256, true, kI4Tab, 10, 2, 157696);
I4_PLAN(1024, true, 3000, 256, false, kI4Tab, 10, 5, 157696);
I4_PLAN(1024, true, 3000, 256, true, kI4Tab, 10, 2, 157696);
I4_PLAN(1024, true, 65, 256, true, kI4Tab, 10, 1, 157696);
I4_PLAN(1024, true, 1, 0, false, kI4Tab, 10, 1, 157696);
#undef I4_PLAN
static_assert(vg::int4_whole_pieces(640) && vg::int4_whole_pieces(1536) && !vg::int4_whole_pieces(544) && !vg::int4_whole_pieces(64),
              "the body of int4_scan_kernel: row bytes a multiple of 128");

// The (node, level) pairs and the batches of a plan, restated: pair_base is contiguous, every node's pairs are levels
// 0..min(level, top when its batch began) in order, every batch starts from the entry point and top level that
// updateEntryPoint (hnsw.go:885-900) leaves after the batches before it.
static void check_plan_pairs(const vg::HnswBuildPlan &p, uint32_t entry, int top)
{
    const int64_t n_old = p.n_old;
    int64_t done = n_old ? n_old : 1, max_pairs = 1, max_b = 1;
    EXPECT(p.pair_base.size() == size_t(p.count) + 1 && p.pair_base[0] == 0);
    if (!n_old && p.count) EXPECT(p.pair_base[1] == 0);  // row 0 of an empty graph: the entry point, no links
    for (const vg::BuildBatch &bt : p.batches) {
        EXPECT(bt.t0 == done && bt.size >= 1 && bt.entry == entry && bt.cur_top == top);
        int64_t npairs = 0;
        for (int64_t t = bt.t0; t < bt.t0 + bt.size; t++) {
            const int64_t i = t - n_old, base = p.pair_base[i];
            const int np = std::min(p.levels[i], bt.cur_top) + 1;
            EXPECT(p.pair_base[i + 1] == base + np);
            for (int l = 0; l < np; l++) EXPECT(p.pair_node[base + l] == uint32_t(t) && p.pair_level[base + l] == l);
            npairs += np;
        }
        for (int64_t t = bt.t0; t < bt.t0 + bt.size; t++)
            if (p.levels[t - n_old] > top) top = p.levels[t - n_old], entry = uint32_t(t);
        EXPECT(bt.npairs == npairs);
        max_pairs = std::max(max_pairs, npairs);
        max_b = std::max(max_b, bt.size);
        done += bt.size;
    }
    EXPECT(done == std::max<int64_t>(n_old + p.count, 1) || p.count == 0);
    EXPECT(int64_t(p.pair_node.size()) == p.pair_base[p.count] && p.pair_level.size() == p.pair_node.size());
    EXPECT(p.max_pairs == max_pairs && p.max_b == max_b);
    EXPECT(p.entry == entry && p.top == top);
}

// vg_build_plan.hpp against the oracle: the batch rule, the levels and level rows, and that an insert plan over [c, n)
// ends where the full plan over [0, n) ends.  M = 2 at n = 1200 is the smallest shape where a new top level appears
// mid-schedule; n = 1 is an empty schedule.
static void check_build_plan()
{
    const int ns[] = {1, 2, 40, 1200}, ms[] = {2, 8, 32}, sched[][2] = {{1, 32}, {64, 16}, {8192, 32}};
    for (int n : ns)
        for (int m : ms)
            for (auto &sc : sched) {
                const int mb = sc[0], gd = sc[1];
                const vg::HnswBuildPlan full = vg::plan_hnsw_build(0, n, m, mb, gd, 0, 0, {});
                std::vector<int32_t> lv(n);
                int64_t rows[63];
                const int top = vgo_hnsw_build_layout(n, m, lv.data(), rows);
                EXPECT(full.top == top && full.levels == lv && full.level_off.size() == size_t(top) + 1);
                for (int l = 0; l < top; l++) EXPECT(full.level_off[l + 1] - full.level_off[l] == rows[l]);
                EXPECT(full.upper_rows == full.level_off[top] && full.total_rows == n + full.upper_rows);
                EXPECT(full.slots.size() == size_t(top) * n);
                for (int l = 0; l < top; l++) {
                    uint32_t next = 0;
                    for (int i = 0; i < n; i++) EXPECT(full.slots[size_t(l) * n + i] == (lv[i] >= l + 1 ? next++ : 0xFFFFFFFFu));
                }
                size_t bi = 0;
                for (int64_t done = 1; done < n; bi++) {
                    const int64_t b = vgo_hnsw_build_batch(done, n, mb, gd);
                    EXPECT(vg::next_batch(done, n, mb, gd) == b);
                    EXPECT(bi < full.batches.size() && full.batches[bi].t0 == done && full.batches[bi].size == b);
                    done += b;
                }
                EXPECT(bi == full.batches.size());
                check_plan_pairs(full, 0, lv[0]);
                for (int c : {1, n / 2, n - 1}) {
                    if (c < 1 || c > n - 1) continue;
                    const vg::HnswBuildPlan head = vg::plan_hnsw_build(0, c, m, mb, gd, 0, 0, {});
                    const vg::HnswBuildPlan tail = vg::plan_hnsw_build(c, n - c, m, mb, gd, head.entry, head.top, head.level_off);
                    check_plan_pairs(tail, head.entry, head.top);
                    EXPECT(tail.entry == full.entry && tail.top == full.top && tail.level_off == full.level_off);
                    EXPECT(tail.total_rows == full.total_rows);
                    for (int l = 0; l < top; l++)  // the new nodes' rows go where a full build puts them
                        for (int i = c; i < n; i++) EXPECT(tail.slots[size_t(l) * (n - c) + (i - c)] == full.slots[size_t(l) * n + i]);
                }
            }
}

int main()
{
    check_build_plan();
    if (g_fail) {
        std::fprintf(stderr, "%d host-only check(s) failed\n", g_fail);
        return 1;
    }
    if (vg_abi_version() != VG_ABI_VERSION) {
        std::printf("libvecgo_hip.so has ABI version %d, the header %d\n", vg_abi_version(), VG_ABI_VERSION);
        return 1;
    }
    std::shared_ptr<Context> ctx;
    try {
        ctx = std::make_shared<Context>(0);
    } catch (const Error &e) {
        std::printf("no usable device: status %d (%s)\n", e.status(), e.what());
        return e.status() == VG_ERR_NO_DEVICE ? 77 : 1;
    }
    std::mt19937 rng(0);

    // ---- ProductQuantizer (pq_test.go) ----------------------------------------------------
    {
        const int dim = 128, m = 8, k = 256;
        ProductQuantizer pq(ctx, dim, m, k);
        EXPECT(!pq.IsTrained());
        auto probe = unit_vectors(rng, 1, dim)[0];
        EXPECT(status_of([&] { pq.Encode(probe); }) == VG_ERR_NOT_TRAINED);  // pq.go:148-150
        auto train = unit_vectors(rng, 1000, dim);
        pq.Train(train);
        EXPECT(pq.IsTrained());
        auto test = unit_vectors(rng, 2, dim);
        auto codes = pq.Encode(test[0]);
        EXPECT(int(codes.size()) == m);
        auto rec = pq.Decode(codes);
        EXPECT(int(rec.size()) == dim);
        double mse = 0;
        for (int i = 0; i < dim; i++) mse += double(test[0][i] - rec[i]) * (test[0][i] - rec[i]);
        EXPECT(mse / dim < 0.5);                                             // pq_test.go:58-71
        EXPECT(std::fabs(pq.CompressionRatio() - double(dim) * 4 / m) < 1e-9);
        const float adc = pq.ComputeAsymmetricDistance(test[1], codes);      // pq_test.go:84-128
        float full = 0;
        for (int i = 0; i < dim; i++) full += (test[1][i] - rec[i]) * (test[1][i] - rec[i]);
        EXPECT(std::fabs(adc - full) <= 1e-3f);
        auto table = pq.BuildDistanceTable(test[1]);
        EXPECT(int(table.size()) == m * k);
        EXPECT(std::fabs(pq.AdcDistance(table, codes) - adc) <= 1e-4f);
        EXPECT(status_of([&] { pq.Encode(std::vector<float>(100)); }) == VG_ERR_DIM_MISMATCH);
        EXPECT(status_of([&] { pq.Decode(std::vector<uint8_t>(3)); }) == VG_ERR_CODE_LENGTH);
        EXPECT(status_of([&] { ProductQuantizer bad(ctx, 100, 7, 256); }) == VG_ERR_INVALID_ARG);  // pq_test.go:130-136
        EXPECT(status_of([&] { ProductQuantizer bad(ctx, 128, 8, 257); }) == VG_ERR_INVALID_ARG);
        // SetCodebooks round trip (pq.go:452-464)
        std::vector<int8_t> cb;
        std::vector<float> sc, of;
        pq.Codebooks(cb, sc, of);
        ProductQuantizer pq2(ctx, dim, m, k);
        pq2.SetCodebooks(cb, sc, of);
        EXPECT(pq2.Encode(test[0]) == codes);
    }

    // ---- RaBitQuantizer (rabitq_test.go) --------------------------------------------------
    {
        const int dim = 128;
        RaBitQuantizer rq(ctx, dim);
        std::uniform_real_distribution<float> ud(-1.f, 1.f);
        std::vector<float> v(dim), q(dim);
        double ss = 0;
        for (auto &x : v) {
            x = ud(rng);
            ss += double(x) * x;
        }
        for (auto &x : q) x = ud(rng);
        auto code = rq.Encode(v);
        EXPECT(int64_t(code.size()) == ((dim + 63) / 64 * 8) + 4);
        float stored;
        std::memcpy(&stored, code.data() + code.size() - 4, 4);
        EXPECT(std::fabs(stored - float(std::sqrt(ss))) < 1e-5f);
        EXPECT(rq.Distance(q, code) >= 0.0f);
        EXPECT(status_of([&] { rq.Encode(std::vector<float>(dim - 1)); }) == VG_ERR_DIM_MISMATCH);
        EXPECT(status_of([&] { rq.Distance(q, std::vector<uint8_t>(5)); }) == VG_ERR_CODE_LENGTH);
    }

    // ---- ScalarQuantizer (quantizer_test.go) ---------------------------------------------------
    {
        quantization::ScalarQuantizer sq(ctx, 3);
        EXPECT(status_of([&] { sq.Encode({1.f, 2.f, 3.f}); }) == VG_ERR_NOT_TRAINED);
        sq.Train({{-1.0f, 0.0f, 1.0f}, {-0.5f, 0.5f, 2.0f}, {-2.0f, 1.0f, 3.0f}});  // quantizer_test.go:8-37
        auto mins = sq.Mins(), maxs = sq.Maxs();
        EXPECT(mins[0] == -2.0f && maxs[0] == -0.5f && mins[2] == 1.0f && maxs[2] == 3.0f);
        quantization::ScalarQuantizer sq4(ctx, 4);                                  // quantizer_test.go:230-271
        sq4.SetBounds({0, 0, 0, 0}, {10, 10, 10, 10});
        auto c1 = sq4.Encode({1, 2, 3, 4}), c2 = sq4.Encode({2, 3, 4, 5});
        std::vector<uint8_t> codes(c1);
        codes.insert(codes.end(), c2.begin(), c2.end());
        std::vector<float> out(2);
        sq4.L2DistanceBatch({1, 2, 3, 4}, codes, 2, out);
        EXPECT(out[0] <= 0.1f && std::fabs(out[1] - 4.0f) <= 0.2f);
        auto dec = sq4.Decode(sq4.Encode({-5.f, 5.f, 20.f, 10.f}));                 // clamping, :148-179
        EXPECT(dec[0] >= -0.01f && dec[2] <= 10.01f && std::fabs(dec[1] - 5.f) <= 10.f / 255.f);
        EXPECT(status_of([&] { sq4.Encode(std::vector<float>(3)); }) == VG_ERR_DIM_MISMATCH);
        EXPECT(sq4.BytesPerDimension() == 1 && sq4.CompressionRatio() == 4.0);
    }

    // ---- Int4Quantizer (int4_test.go) ------------------------------------------------------------
    {
        quantization::Int4Quantizer odd(ctx, 3);
        odd.Train({{0.1f, 0.5f, 0.9f}});                                   // int4_test.go:50-66
        auto enc = odd.Encode({0.1f, 0.5f, 0.9f});
        EXPECT(enc.size() == 2 && (enc[1] & 0x0F) == 0);
        auto dec = odd.Decode(enc);
        EXPECT(dec.size() == 3 && std::fabs(dec[0] - 0.1f) <= 0.1f && std::fabs(dec[1] - 0.5f) <= 0.1f &&
               std::fabs(dec[2] - 0.9f) <= 0.1f);
        quantization::Int4Quantizer iq(ctx, 4);
        iq.SetParams({0, 0, 0, 0}, {1, 1, 1, 1});
        auto c = iq.Encode({0.0f, 1.0f, 0.5f, 2.0f});                      // 0, 15, round(7.5) = 8, clamp -> 15
        EXPECT(c.size() == 2 && c[0] == 0x0F && c[1] == 0x8F);
        const float d1 = iq.L2Distance({0.0f, 1.0f, 8.0f / 15.0f, 1.0f}, c);
        std::vector<float> out(1);
        iq.L2DistanceBatch({0.0f, 1.0f, 8.0f / 15.0f, 1.0f}, c, 1, out);
        EXPECT(d1 < 1e-9f && out[0] < 1e-9f);
        EXPECT(status_of([&] { iq.Encode(std::vector<float>(3)); }) == VG_ERR_DIM_MISMATCH);
        EXPECT(iq.BytesPerDimension() == 0);
    }

    // ---- kmeans (kmeans_test.go) --------------------------------------------------------------
    {
        std::normal_distribution<float> nd;
        std::vector<float> x;
        for (int i = 0; i < 100; i++)
            for (int d = 0; d < 4; d++) x.push_back(nd(rng) * 0.1f + (i < 50 ? 0.f : 10.f));
        auto c = kmeans::TrainKMeans(*ctx, x, 4, 2, distance::Metric::L2, 10, 3);
        EXPECT(c.size() == 8);
        const float m0 = (c[0] + c[1] + c[2] + c[3]) / 4, m1 = (c[4] + c[5] + c[6] + c[7]) / 4;
        EXPECT(std::fabs(std::min(m0, m1)) < 0.5f && std::fabs(std::max(m0, m1) - 10.f) < 0.5f);
        EXPECT(kmeans::TrainKMeans(*ctx, std::vector<float>(4, 1.f), 4, 2, distance::Metric::L2, 10).empty());
        EXPECT(status_of([&] { kmeans::TrainKMeans(*ctx, x, 4, 2, distance::Metric::Hamming, 10); }) == VG_ERR_UNSUPPORTED);
        std::vector<float> cents = {0, 0, 1, 1, 5, 5, 10, 10};
        auto near = kmeans::FindClosestCentroids(*ctx, {0.9f, 0.9f}, cents, 2, 2, distance::Metric::L2);
        EXPECT(near.size() == 2 && near[0] == 1 && near[1] == 0);
        EXPECT(kmeans::AssignPartition(*ctx, {9.f, 9.f}, cents, 2, distance::Metric::L2) == 3);
    }

    // ---- distance.Provider -----------------------------------------------------------------------
    {
        std::vector<float> a = {1, 2, 3}, b = {4, 5, 6};
        float out = 0;
        distance::Provider(distance::Metric::L2)(*ctx, a.data(), b.data(), 3, 1, &out);
        EXPECT(out == 27.0f);  // floats_test.go:61
        distance::Provider(distance::Metric::Cosine)(*ctx, a.data(), b.data(), 3, 1, &out);
        EXPECT(out == 32.0f);  // floats_test.go:17
        EXPECT(status_of([&] { distance::Provider(distance::Metric::Hamming); }) == VG_ERR_UNSUPPORTED);
        // distance_test.go:119-152 TestMetric: String() of every metric and of an unknown one, Provider's errors
        EXPECT(distance::String(distance::Metric::L2) == "L2" && distance::String(distance::Metric::Cosine) == "Cosine");
        EXPECT(distance::String(distance::Metric::Dot) == "Dot" && distance::String(distance::Metric::Hamming) == "Hamming");
        EXPECT(distance::String(static_cast<distance::Metric>(99)) == "Unknown(99)");
        EXPECT(status_of([&] { distance::Provider(static_cast<distance::Metric>(99)); }) == VG_ERR_UNSUPPORTED);
    }

    // ---- flat segment: exact search and PQ search, vs the oracle ------------------------------
    {
        const int n = 4000, dim = 128, k = 10, nq = 5;
        std::normal_distribution<float> nd;
        std::vector<float> base(size_t(n) * dim), q(size_t(nq) * dim);
        for (auto &x : base) x = nd(rng);
        for (auto &x : q) x = nd(rng);
        Segment seg(ctx, n, dim, distance::Metric::L2);
        seg.SetVectors(base.data());
        auto r = seg.SearchFlat(q.data(), nq, k);
        for (int i = 0; i < nq; i++) {
            uint32_t eid[k];
            float esc[k];
            vgo_flat_search_f32(base.data(), n, dim, VGO_METRIC_L2, q.data() + size_t(i) * dim, k, eid, esc);
            EXPECT(std::memcmp(eid, r.ids.data() + size_t(i) * k, sizeof eid) == 0);
            EXPECT(std::memcmp(esc, r.scores.data() + size_t(i) * k, sizeof esc) == 0);
        }
        // the opt-in bfloat16 nomination filter: same ids, same fp32 scores
        {
            const int nq2 = 96;
            std::vector<float> q2(size_t(nq2) * dim);
            for (auto &x : q2) x = nd(rng);
            auto plain = seg.SearchFlat(q2.data(), nq2, k);
            seg.EnableBF16Filter(true);
            auto filtered = seg.SearchFlat(q2.data(), nq2, k);
            seg.EnableBF16Filter(false);
            EXPECT(plain.ids == filtered.ids);
            EXPECT(std::memcmp(plain.scores.data(), filtered.scores.data(), plain.scores.size() * sizeof(float)) == 0);
        }
        // flat/pq_test.go:17-93: the zero query finds the zero vector with a small score
        auto pq = std::make_shared<ProductQuantizer>(ctx, dim, 16, 256);
        std::vector<float> with_zero(base);
        std::fill(with_zero.begin() + 7 * dim, with_zero.begin() + 8 * dim, 0.0f);
        pq->TrainFlat(with_zero.data(), 1000, 20, 1);
        std::vector<uint8_t> codes(size_t(n) * 16);
        pq->EncodeBatch(with_zero.data(), n, codes.data());
        Segment pseg(ctx, n, dim, distance::Metric::L2);
        pseg.SetVectors(with_zero.data());
        pseg.SetPQCodes(pq, codes.data());
        std::vector<float> zero(dim, 0.0f);
        auto pr = pseg.SearchPQ(zero.data(), 1, 10);
        bool found = false;
        for (int i = 0; i < 10; i++) found |= pr.ids[i] == 7u;
        EXPECT(found);
        auto rr = pseg.Rerank(zero.data(), 1, pr.ids.data(), 10, 1);
        EXPECT(rr.ids[0] == 7u && rr.scores[0] == 0.0f);

        // IVF partitions (flat/segment.go:727-749): four row ranges with the first rows of each as
        // centroids; NProbes 2 scans the two closest partitions only — vs the oracle's restatement
        const int parts = 4;
        std::vector<uint32_t> off = {0, 1000, 1900, 3100, 4000};
        std::vector<float> cent(size_t(parts) * dim);
        for (int p = 0; p < parts; p++) std::copy_n(base.data() + size_t(off[p]) * dim, dim, cent.data() + size_t(p) * dim);
        seg.SetPartitions(cent.data(), off.data(), parts);
        auto probed = seg.SearchProbed(q.data(), nq, k, 2, VG_SCAN_F32);
        vgo_flat_segment os{};
        os.n = n; os.dim = dim; os.metric = VGO_METRIC_L2; os.base = base.data();
        os.num_partitions = parts; os.centroids = cent.data(); os.part_offsets = off.data();
        for (int i = 0; i < nq; i++) {
            uint32_t eid[k];
            float esc[k];
            EXPECT(vgo_flat_segment_search(&os, q.data() + size_t(i) * dim, k, 2, eid, esc) == k);
            EXPECT(std::memcmp(eid, probed.ids.data() + size_t(i) * k, sizeof eid) == 0);
            EXPECT(std::memcmp(esc, probed.scores.data() + size_t(i) * k, sizeof esc) == 0);
        }
    }

    // ---- BinaryQuantizer (binary_test.go) ---------------------------------------------------
    {
        vecgo::quantization::BinaryQuantizer bq(ctx, 128);
        std::vector<float> v(128);
        for (int i = 0; i < 128; i++) v[i] = i % 2 == 0 ? 1.0f : -1.0f;
        auto w = bq.EncodeUint64(v);                                         // binary_test.go:9-39
        EXPECT(w.size() == 2 && w[0] == 0x5555555555555555ull && w[1] == 0x5555555555555555ull);
        vecgo::quantization::BinaryQuantizer b4(ctx, 4);
        b4.Train({{1, 2, 3, 4}, {5, 6, 7, 8}});                              // binary_test.go:41-63
        EXPECT(b4.IsTrained() && b4.Threshold() == 4.5f);
        EXPECT(status_of([&] { b4.Train({}); }) == VG_ERR_INVALID_ARG);
        vecgo::quantization::BinaryQuantizer b8(ctx, 8);
        b8.WithThreshold(0.5f);                                              // binary_test.go:64-100
        auto code = b8.Encode({0.1f, 0.9f, 0.5f, 0.4f, 0.6f, 0.3f, 0.8f, 0.2f});
        EXPECT(code[0] == 0b01010110);
        auto dec = b8.Decode(code);
        EXPECT(dec[0] == 0.0f && dec[1] == 1.0f && dec[2] == 1.0f && dec[3] == 0.0f);
        std::vector<float> a(128, 1.0f), b(128, 1.0f);
        for (int i = 0; i < 10; i++) b[i * 7] = -1.0f;
        EXPECT(bq.ComputeHammingDistance(a, bq.EncodeUint64(b)) == 10);      // binary_test.go:102-123 shape
        EXPECT(bq.BytesTotal() == 16 && bq.CompressionRatio() == 32.0f);
        EXPECT(status_of([&] { bq.Encode(std::vector<float>(3)); }) == VG_ERR_DIM_MISMATCH);
    }

    // ---- NormalizeL2InPlace (distance_test.go) ----------------------------------------------
    {
        std::vector<float> v{3.0f, 4.0f};
        EXPECT(vecgo::distance::NormalizeL2InPlace(*ctx, v));
        EXPECT(std::fabs(v[0] - 0.6f) < 1e-6f && std::fabs(v[1] - 0.8f) < 1e-6f);
        std::vector<float> z{0.0f, 0.0f, 0.0f}, e;
        EXPECT(!vecgo::distance::NormalizeL2InPlace(*ctx, z) && z[0] == 0.0f);
        EXPECT(!vecgo::distance::NormalizeL2InPlace(*ctx, e));
    }

    // ---- OptimizedProductQuantizer (opq_test.go) --------------------------------------------
    {
        const int dim = 32, m = 8;
        vecgo::quantization::OptimizedProductQuantizer opq(ctx, dim, m, 16, 3);
        EXPECT(!opq.IsTrained());
        EXPECT(status_of([&] { opq.Encode(std::vector<float>(dim)); }) == VG_ERR_NOT_READY);   // "not trained" opq_test.go:202-221
        EXPECT(status_of([&] { vecgo::quantization::OptimizedProductQuantizer bad(ctx, 30, 8, 16, 1); }) == VG_ERR_INVALID_ARG);
        auto train = unit_vectors(rng, 400, dim);
        opq.Train(train);                                                    // opq_test.go:26-54
        EXPECT(opq.IsTrained());
        auto codes = opq.Encode(train[0]);
        EXPECT(int(codes.size()) == m && opq.BytesPerVector() == m);
        auto rec = opq.Decode(codes);
        EXPECT(int(rec.size()) == dim);
        EXPECT(std::fabs(opq.CompressionRatio() - 16.0) < 0.1);
        int bs = 0, nb = 0;                                                  // opq_test.go:56-99: R R^T = I
        auto rot = opq.Rotations(bs, nb);
        EXPECT(bs * nb == dim);
        for (int b = 0; b < nb; b++)
            for (int i = 0; i < bs; i++)
                for (int j = 0; j < bs; j++) {
                    float s = 0;
                    for (int k2 = 0; k2 < bs; k2++) s += rot[(size_t(b) * bs + i) * bs + k2] * rot[(size_t(b) * bs + j) * bs + k2];
                    EXPECT(std::fabs(s - (i == j ? 1.0f : 0.0f)) < 0.1f);
                }
        const float self = opq.ComputeAsymmetricDistance(train[0], codes);   // opq_test.go:101-131
        const float other = opq.ComputeAsymmetricDistance(train[1], codes);
        EXPECT(other > 0.0f && self < other);
    }

    // ---- hnsw build + search (hnsw_test.go:43-60: 1000 x 16, M = 8, EF = 200 -> precision >= 0.99) ----
    {
        const int n = 1000, dim = 16, k = 10, nq = 50;
        std::uniform_real_distribution<float> ud(0.f, 1.f);
        std::vector<float> base(size_t(n) * dim), q(size_t(nq) * dim);
        for (auto &x : base) x = ud(rng);
        for (auto &x : q) x = ud(rng);
        Segment seg(ctx, n, dim, distance::Metric::L2);
        seg.SetVectors(base.data());
        seg.BuildHNSW(8, 200, 16, 32);
        auto got = seg.SearchHNSW(q.data(), nq, k, 200);
        auto want = seg.SearchFlat(q.data(), nq, k);
        int hit = 0;
        for (int i = 0; i < nq; i++)
            for (int a = 0; a < k; a++)
                for (int b = 0; b < k; b++) hit += got.ids[size_t(i) * k + a] == want.ids[size_t(i) * k + b];
        EXPECT(hit >= int(0.99 * nq * k));
        // hnsw.BruteSearch (hnsw.go:2021-2101) and searchBitmap (:2240-2263) vs the oracle's replay of the same heaps,
        // on a tie-heavy copy of the rows (two decimals of a 16-dim uniform: equal distances do occur)
        std::vector<float> coarse(base);
        for (auto &x : coarse) x = std::floor(x * 3.0f);
        Segment tie(ctx, n, dim, distance::Metric::L2);
        tie.SetVectors(coarse.data());
        std::vector<float> cq(q);
        for (auto &x : cq) x = std::floor(x * 3.0f);
        std::vector<uint8_t> mask((n + 7) / 8);
        for (auto &b : mask) b = uint8_t(rng());
        std::vector<uint32_t> none(size_t(n), 0xFFFFFFFFu);
        vgo_hnsw_graph og{};
        og.n = n, og.dim = dim, og.metric = VGO_METRIC_L2, og.base = coarse.data(), og.m0 = 1, og.l0 = none.data();
        for (int mode = 0; mode < 2; mode++)
            for (int masked = 0; masked < 2; masked++) {
                auto br = tie.SearchHNSWBrute(cq.data(), nq, k, mode, masked ? mask.data() : nullptr);
                for (int i = 0; i < nq; i++) {
                    uint32_t eid[k];
                    float esc[k];
                    const int r = vgo_hnsw_brute_search(&og, cq.data() + size_t(i) * dim, k, mode, masked ? mask.data() : nullptr, eid, esc);
                    EXPECT(r == k);
                    EXPECT(std::memcmp(eid, br.ids.data() + size_t(i) * k, sizeof eid) == 0);
                    EXPECT(std::memcmp(esc, br.scores.data() + size_t(i) * k, sizeof esc) == 0);
                }
            }
    }

    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("host mirror: all checks passed\n");
    return 0;
}
