// guide_check.cpp — the host side of the library guide (plan_guide, guide_plan_report: csrc/host_plan.hpp,
// csrc/plan_report.hpp), checked without HIP under -fsanitize=address,undefined: the sweep of
// tests/test_guide_host.py over in_dim x widths x layers x activation x rows —
//   * the grid covers the rows exactly once, 32 rows a block;
//   * a refusal occurs exactly when a stated limit says so, in the order of DAD_GD_REFUSALS, and a plan that is not
//     refused fits one CU's LDS, with the padding whole 32-column tiles;
//   * the report carries the plan field by field; bad shapes are refused with a message.
// Built and run by tests/test_guide_host.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dynamics_aware_diffusion_amd/csrc/plan_report.hpp"

using namespace dadhost;

static int g_failures = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            if (++g_failures <= 40) {                                                     \
                fprintf(stderr, "CHECK failed %s:%d: %s — ", __FILE__, __LINE__, #cond);  \
                fprintf(stderr, __VA_ARGS__);                                             \
                fprintf(stderr, "\n");                                                    \
            }                                                                             \
        }                                                                                 \
    } while (0)

// the stated limits, written out independently of plan_guide
static int expected(int in_dim, const std::vector<int>& w, int act, int td, size_t* lds) {
    const int L = (int)w.size();
    *lds = 0;
    if (L < 2 || L > 4) return DAD_GD_BAD_LAYERS;
    for (int v : w) if (v < 1 || v > 512) return DAD_GD_BAD_WIDTH;
    if (act < 0 || act > 2) return DAD_GD_BAD_ACT;
    if (in_dim < 1 || in_dim > td) return DAD_GD_BAD_IN_DIM;
    if (w.back() != 1) return DAD_GD_BAD_LAST;
    size_t cols = (size_t)(in_dim + 31) / 32 * 32;
    for (int i = 0; i + 1 < L; ++i) cols += (size_t)((w[i] + 31) / 32 * 32) * (act == DAD_GD_MISH ? 2 : 1);
    *lds = cols * 33 * sizeof(float);
    return *lds > 160 * 1024 ? DAD_GD_BAD_LDS : DAD_GD_OK;
}

int main() {
    const int in_dims[] = {1, 6, 39, 67};
    const int widths[] = {1, 16, 32, 33, 256, 512, 513};
    const int rows[][2] = {{1, 8}, {4, 8}, {3, 11}, {256, 32}};      // B * H = 8, 32, 33, 8192
    long plans = 0, refused = 0;
    std::vector<std::vector<int>> nets;
    for (int a : widths) {
        nets.push_back({a});                                          // one layer: refused
        nets.push_back({a, 1});
        for (int b : widths) {
            nets.push_back({a, b});                                   // last width b: refused unless 1
            nets.push_back({a, b, 1});
            for (int c : {1, 33, 512, 513}) nets.push_back({a, b, c, 1});
        }
    }
    nets.push_back({16, 16, 16, 16, 1});                              // five layers
    for (const auto& w : nets)
        for (int in_dim : in_dims)
            for (int act = -1; act <= 3; ++act)
                for (const auto& bh : rows)
                    for (int td : {in_dim, in_dim + 5, in_dim - 1}) {
                        if (td < 1) continue;
                        size_t lds = 0;
                        const int want = expected(in_dim, w, act, td, &lds);
                        const GuidePlan q = plan_guide(in_dim, w.data(), (int)w.size(), act, bh[0], bh[1], td);
                        ++plans;
                        refused += q.refused != DAD_GD_OK;
                        CHECK(q.refused == want, "in_dim %d, %zu layers (first %d), act %d, td %d: refused %d, expected %d", in_dim,
                              w.size(), w[0], act, td, q.refused, want);
                        const long n = (long)bh[0] * bh[1];
                        CHECK(q.rows_per_block == 32 && (long)q.gx * 32 >= n && ((long)q.gx - 1) * 32 < n, "grid %u for %ld rows", q.gx, n);
                        CHECK(q.threads == 256, "threads %d", q.threads);
                        if (q.refused == DAD_GD_OK) {
                            CHECK(q.lds_bytes == lds && q.lds_bytes <= dad::kLdsBytes, "lds %zu, expected %zu", q.lds_bytes, lds);
                            CHECK(q.padded[0] % 32 == 0 && q.padded[0] >= in_dim && q.padded[0] < in_dim + 32, "padded in %d", q.padded[0]);
                            for (size_t i = 0; i + 1 < w.size(); ++i)
                                CHECK(q.padded[i + 1] % 32 == 0 && q.padded[i + 1] >= w[i] && q.padded[i + 1] < w[i] + 32, "padded[%zu] = %d",
                                      i + 1, q.padded[i + 1]);
                            for (size_t i = w.size(); i < 4; ++i) CHECK(q.padded[i] == 0, "padded[%zu] = %d of a layer that is not there", i, q.padded[i]);
                        }
                        // the report says the same, field by field
                        int32_t out[DAD_GD_INTS];
                        std::memset(out, 0xff, sizeof out);
                        CHECK(guide_plan_report(in_dim, w.data(), (int)w.size(), act, bh[0], bh[1], td, out) == DAD_OK, "report: %s", g_err);
                        CHECK(out[DAD_GD_REFUSED] == q.refused && out[DAD_GD_GX] == (int32_t)q.gx && out[DAD_GD_LAYERS] == (int)w.size() &&
                              out[DAD_GD_PADDED_IN] == q.padded[0] && out[DAD_GD_PADDED_1] == q.padded[1] && out[DAD_GD_PADDED_2] == q.padded[2] &&
                              out[DAD_GD_PADDED_3] == q.padded[3] && out[DAD_GD_ROWS_PER_BLOCK] == 32 && out[DAD_GD_THREADS] == 256 &&
                              out[DAD_GD_LDS_BYTES] == (int32_t)q.lds_bytes, "the report differs from the plan");
                        if (q.refused != DAD_GD_OK) CHECK(std::strlen(guide_refusal(q.refused)) > 0, "refusal %d has no message", q.refused);
                    }
    // shapes every entry point refuses before it plans
    int32_t out[DAD_GD_INTS];
    const int w2[] = {16, 1};
    for (const auto& bad : {std::vector<int>{0, 8, 6}, {3, 0, 6}, {3, 8, 0}, {-1, 8, 6}, {1 << 20, 1 << 10, 8}}) {
        CHECK(guide_plan_report(4, w2, 2, DAD_GD_TANH, bad[0], bad[1], bad[2], out) == DAD_E_INVALID, "shape %d %d %d", bad[0], bad[1], bad[2]);
        CHECK(std::strlen(g_err) > 0, "no message");
    }
    CHECK(plan_guide(4, nullptr, 2, DAD_GD_TANH, 1, 8, 6).refused == DAD_GD_BAD_LAYERS, "null widths");
    CHECK(sizeof(kReportLayouts) / sizeof(kReportLayouts[0]) >= 11, "the guide's row of layouts");

    if (g_failures) {
        fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    printf("guide host logic ok: %ld plans, %ld refused\n", plans, refused);
    return 0;
}
