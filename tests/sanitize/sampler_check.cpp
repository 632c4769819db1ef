// sampler_check.cpp — the host side of dad_sampler_step / dad_sampler_loop (csrc/host_plan.hpp), checked without HIP
// under -fsanitize=address,undefined:
//   * ancestral_coef reproduces the five schedule entries it is given and the two expf values dad_denoise_step has
//     always formed from the log variance (sigma masked at t == 0), with both guide terms where they belong;
//   * check_sampler_steps refuses a t outside the schedule (DAD_E_RANGE), every non-finite coefficient, a negative
//     sigma, n_steps < 1 and a null array (DAD_E_INVALID), names the step, and accepts what the builder makes;
//   * sampler_steps_hash (FNV-1a over the array's bytes) distinguishes any single changed field of any step, the
//     order of two steps and the number of steps, and is a function of the bytes alone.
// Built and run by tests/test_sampler_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "../../dynamics_aware_diffusion_amd/csrc/host_plan.hpp"

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

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// a cosine-like schedule's five entries at t of T, as floats (the values only need to be distinct and finite)
static void entries(int t, int T, float e[5]) {
    const double ab = std::cos((t + 1.0) / (T + 1.0) * 1.5) * std::cos((t + 1.0) / (T + 1.0) * 1.5);
    const double ap = t == 0 ? 1.0 : std::cos((double)t / (T + 1.0) * 1.5) * std::cos((double)t / (T + 1.0) * 1.5);
    const double beta = 1.0 - ab / ap;
    e[0] = (float)std::sqrt(1.0 / ab);
    e[1] = (float)std::sqrt(1.0 / ab - 1.0);
    e[2] = (float)(beta * std::sqrt(ap) / (1.0 - ab));
    e[3] = (float)((1.0 - ap) * std::sqrt(1.0 - beta) / (1.0 - ab));
    e[4] = (float)std::log(std::max(beta * (1.0 - ap) / (1.0 - ab), 1e-20));
}

static float* field(dad_sampler_coef& s, int k) {
    float* const f[7] = {&s.c_recip, &s.c_recipm1, &s.guide_x0, &s.coef_x0, &s.coef_xt, &s.guide_mean, &s.sigma};
    return f[k];
}

int main() {
    const int T = 20;
    std::vector<dad_sampler_coef> steps;
    // ---- the ancestral builder -------------------------------------------------------------------------------
    for (int t = T - 1; t >= 0; --t) {
        float e[5];
        entries(t, T, e);
        const dad_sampler_coef s = ancestral_coef(t, e[0], e[1], e[2], e[3], e[4]);
        CHECK(s.t == t, "t = %d", s.t);
        CHECK(bits(s.c_recip) == bits(e[0]) && bits(s.c_recipm1) == bits(e[1]), "t %d: the x0 scalars", t);
        CHECK(bits(s.coef_x0) == bits(e[2]) && bits(s.coef_xt) == bits(e[3]), "t %d: the mean coefficients", t);
        CHECK(bits(s.guide_mean) == bits(expf(e[4])), "t %d: guide_mean %g is not expf(log_var)", t, (double)s.guide_mean);
        CHECK(bits(s.sigma) == bits(t == 0 ? 0.0f : expf(0.5f * e[4])), "t %d: sigma %g", t, (double)s.sigma);
        CHECK(bits(s.guide_x0) == 0u, "t %d: the ancestral step shifts x0 by %g", t, (double)s.guide_x0);
        steps.push_back(s);
    }
    CHECK(steps.back().sigma == 0.0f && steps[0].sigma > 0.0f, "the mask at t == 0");
    const int n = (int)steps.size();

    // ---- validation ------------------------------------------------------------------------------------------
    CHECK(check_sampler_steps(steps.data(), n, T) == DAD_OK, "the builder's steps are refused: %s", g_err);
    CHECK(check_sampler_steps(steps.data(), 1, T) == DAD_OK, "one step is refused");
    CHECK(check_sampler_steps(steps.data(), 0, T) == DAD_E_INVALID, "n_steps = 0");
    CHECK(check_sampler_steps(steps.data(), -3, T) == DAD_E_INVALID, "n_steps < 0");
    CHECK(check_sampler_steps(nullptr, 1, T) == DAD_E_INVALID, "a null array");
    CHECK(check_sampler_steps(steps.data(), n, T - 1) == DAD_E_RANGE, "t = T - 1 against a schedule of T - 1");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int at : {0, n / 2, n - 1}) {
        for (int bad_t : {-1, T, T + 100, std::numeric_limits<int>::min()}) {
            std::vector<dad_sampler_coef> v = steps;
            v[at].t = bad_t;
            CHECK(check_sampler_steps(v.data(), n, T) == DAD_E_RANGE, "t = %d at step %d", bad_t, at);
        }
        for (int k = 0; k < 7; ++k)
            for (float bad : {nan, inf, -inf}) {
                std::vector<dad_sampler_coef> v = steps;
                *field(v[at], k) = bad;
                CHECK(check_sampler_steps(v.data(), n, T) == DAD_E_INVALID, "field %d = %g at step %d", k, (double)bad, at);
                char want[32];
                snprintf(want, sizeof want, "step %d", at);
                CHECK(std::strstr(g_err, want) != nullptr, "the message '%s' does not name step %d", g_err, at);
            }
        std::vector<dad_sampler_coef> v = steps;
        v[at].sigma = -1e-30f;
        CHECK(check_sampler_steps(v.data(), n, T) == DAD_E_INVALID, "a negative sigma at step %d", at);
        v[at].sigma = 0.0f;
        v[at].coef_x0 = -2.0f; v[at].coef_xt = -0.5f; v[at].guide_x0 = -1.0f;     // only sigma has a sign rule
        CHECK(check_sampler_steps(v.data(), n, T) == DAD_OK, "negative coefficients other than sigma");
    }

    // ---- the hash --------------------------------------------------------------------------------------------
    const uint64_t h0 = sampler_steps_hash(steps.data(), n);
    {
        std::vector<dad_sampler_coef> copy = steps;                  // a function of the bytes, not of the address
        CHECK(sampler_steps_hash(copy.data(), n) == h0, "the hash depends on the address");
        const unsigned char abc[3] = {'a', 'b', 'c'};                // FNV-1a's published test vector
        CHECK(fnv1a_bytes(abc, 3) == 0xe71fa2190541574bull, "fnv1a(\"abc\") = %llx", (unsigned long long)fnv1a_bytes(abc, 3));
        CHECK(fnv1a_bytes(abc, 0) == 0xcbf29ce484222325ull, "fnv1a of nothing");
    }
    std::set<uint64_t> seen{h0};
    for (int at = 0; at < n; ++at) {
        for (int k = -1; k < 7; ++k) {
            std::vector<dad_sampler_coef> v = steps;
            if (k < 0) v[at].t = (v[at].t + 1) % T;
            else *field(v[at], k) = std::nextafterf(*field(v[at], k), 10.0f);       // one ulp
            const uint64_t h = sampler_steps_hash(v.data(), n);
            CHECK(seen.insert(h).second, "step %d field %d: the hash %llx repeats", at, k, (unsigned long long)h);
        }
        std::vector<dad_sampler_coef> v = steps;
        v[at].guide_x0 = -0.0f;                                                     // bytes, not values
        CHECK(seen.insert(sampler_steps_hash(v.data(), n)).second, "step %d: -0 hashes as +0", at);
    }
    for (int k = 1; k < n; ++k) CHECK(seen.insert(sampler_steps_hash(steps.data(), k)).second, "the first %d steps hash as another set", k);
    {
        std::vector<dad_sampler_coef> v = steps;
        std::swap(v[0], v[1]);
        CHECK(seen.insert(sampler_steps_hash(v.data(), n)).second, "two steps swapped hash the same");
    }

    if (g_failures) {
        fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    printf("sampler host logic ok: %d steps, %zu distinct hashes\n", n, seen.size());
    return 0;
}
