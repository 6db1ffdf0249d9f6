// lsap_check.cpp -- stand-alone check of rac_lsap_host (racformer_amd/csrc/lsap_host.cpp), host code only:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/lsap_check.cpp racformer_amd/csrc/lsap_host.cpp -o /tmp/lsap_check && /tmp/lsap_check
// Seeded random and degenerate problems (constant costs, duplicate rows, +-100 entries, G = 0 / 1 / Q / Q + 3, strided and
// transposed layouts); every solution must be a valid matching that carries its own optimality certificate in float64:
//     u_g + v_q <= c(g, q) + 1e-9 everywhere, equality on matched pairs, and on the side that has spare entries the duals are
//     <= 0 (queries; >= is impossible) and exactly 0 where unmatched
// which bounds every other assignment's total from below by this one's.  Small problems are also checked against brute force.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <algorithm>
#include <random>
#include <vector>

extern "C" int rac_lsap_host(const float *cost, int64_t gt_stride, int64_t query_stride, int num_gt, int num_query,
                             int32_t *matched_query, int32_t *matched_gt, double *u, double *v, int64_t *steps);

void rac_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
}

static int g_failed = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            fprintf(stderr, "FAIL %s: ", what); \
            fprintf(stderr, __VA_ARGS__);      \
            fputc('\n', stderr);               \
            ++g_failed;                        \
            return;                            \
        }                                      \
    } while (0)

static double brute(const std::vector<float> &c, int G, int Q)
{
    // minimum over injections of the smaller side into the larger one (small sizes only)
    const int nr = std::min(G, Q), nc = std::max(G, Q);
    std::vector<int> cols(nc);
    for (int j = 0; j < nc; ++j)
        cols[j] = j;
    double best = INFINITY;
    // permutations of the columns, first nr entries used (redundant but tiny)
    std::sort(cols.begin(), cols.end());
    do {
        double t = 0;
        for (int i = 0; i < nr; ++i)
            t += G <= Q ? (double)c[(size_t)i * Q + cols[i]] : (double)c[(size_t)cols[i] * Q + i];
        best = std::min(best, t);
    } while (std::next_permutation(cols.begin(), cols.end()));
    return best;
}

// c: dense [G][Q]; layout 0: as is, 1: transposed storage [Q][G], 2: padded rows (pitch Q + 5)
static void check(const char *what, const std::vector<float> &c, int G, int Q, int layout)
{
    std::vector<float> store;
    int64_t gs, qs;
    if (layout == 0) {
        store = c; gs = Q; qs = 1;
    } else if (layout == 1) {
        store.assign((size_t)G * Q, 0.f);
        for (int g = 0; g < G; ++g)
            for (int q = 0; q < Q; ++q)
                store[(size_t)q * G + g] = c[(size_t)g * Q + q];
        gs = 1; qs = G;
    } else {
        store.assign((size_t)G * (Q + 5), NAN);       // the pad is never read
        for (int g = 0; g < G; ++g)
            for (int q = 0; q < Q; ++q)
                store[(size_t)g * (Q + 5) + q] = c[(size_t)g * Q + q];
        gs = Q + 5; qs = 1;
    }
    std::vector<int32_t> mq(G), mg(Q);
    std::vector<double> u(G), v(Q);
    int64_t steps = -1;
    const int rc = rac_lsap_host(store.data(), gs, qs, G, Q, mq.data(), mg.data(), u.data(), v.data(), &steps);
    CHECK(rc == 0, "rc = %d", rc);
    const int n = std::min(G, Q);
    int matched = 0;
    double total = 0, dual = 0;
    for (int g = 0; g < G; ++g) {
        CHECK(mq[g] >= -1 && mq[g] < Q, "matched_query[%d] = %d", g, mq[g]);
        if (mq[g] >= 0) {
            CHECK(mg[mq[g]] == g, "matched_gt[%d] = %d, expected %d", mq[g], mg[mq[g]], g);
            ++matched;
            total += (double)c[(size_t)g * Q + mq[g]];
        }
    }
    int back = 0;
    for (int q = 0; q < Q; ++q) {
        CHECK(mg[q] >= -1 && mg[q] < G, "matched_gt[%d] = %d", q, mg[q]);
        back += mg[q] >= 0;
    }
    CHECK(matched == n && back == n, "%d boxes and %d queries matched, expected %d", matched, back, n);
    for (int g = 0; g < G; ++g)
        for (int q = 0; q < Q; ++q) {
            const double slack = (double)c[(size_t)g * Q + q] - u[g] - v[q];
            CHECK(slack >= -1e-9, "dual infeasible at (%d, %d): slack %.3e", g, q, slack);
            if (mq[g] == q)
                CHECK(fabs(slack) <= 1e-9, "matched pair (%d, %d) has slack %.3e", g, q, slack);
        }
    for (int g = 0; g < G; ++g) {
        dual += u[g];
        if (G > Q) {
            CHECK(u[g] <= 1e-9, "u[%d] = %.3e > 0 on the spare side", g, u[g]);
            if (mq[g] < 0)
                CHECK(u[g] == 0.0, "unmatched box %d has u = %.3e", g, u[g]);
        }
    }
    for (int q = 0; q < Q; ++q) {
        dual += v[q];
        if (G <= Q) {
            CHECK(v[q] <= 1e-9, "v[%d] = %.3e > 0 on the spare side", q, v[q]);
            if (mg[q] < 0)
                CHECK(v[q] == 0.0, "unmatched query %d has v = %.3e", q, v[q]);
        }
    }
    CHECK(fabs(total - dual) <= 1e-9 * std::max(1.0, fabs(total)), "primal %.12g != dual %.12g", total, dual);
    CHECK(steps >= n && steps <= (int64_t)n * (n + 1) / 2 + (n == 0), "steps = %ld for n = %d", (long)steps, n);
    if (std::max(G, Q) <= 7 && n >= 1) {
        const double b = brute(c, G, Q);
        CHECK(fabs(b - total) <= 1e-9 * std::max(1.0, fabs(b)), "total %.12g, brute force %.12g", total, b);
    }
}

static void all_layouts(const char *what, const std::vector<float> &c, int G, int Q)
{
    for (int layout = 0; layout < 3; ++layout)
        check(what, c, G, Q, layout);
}

int main()
{
    std::mt19937 rng(20240607);
    std::uniform_real_distribution<float> uni(-3.f, 8.f);
    int problems = 0;
    const int Qs[] = {1, 2, 5, 7, 64, 70, 130};
    for (int Q : Qs) {
        const int Gs[] = {0, 1, Q / 2, Q, Q + 3};
        for (int G : Gs) {
            std::vector<float> c((size_t)G * Q);
            // random
            for (int rep = 0; rep < 3; ++rep) {
                for (float &x : c)
                    x = uni(rng);
                all_layouts("random", c, G, Q);
                ++problems;
            }
            // constant
            std::fill(c.begin(), c.end(), 1.25f);
            all_layouts("constant", c, G, Q);
            // duplicate rows: every box the same row
            for (int g = 0; g < G; ++g)
                for (int q = 0; q < Q; ++q)
                    c[(size_t)g * Q + q] = (float)((q * 37) % 11) * 0.5f;
            all_layouts("duplicate rows", c, G, Q);
            // few distinct values with +-100 entries (what nan_to_num leaves)
            for (float &x : c) {
                const unsigned r = rng() % 10;
                x = r == 0 ? 100.f : (r == 1 ? -100.f : (float)(rng() % 4));
            }
            all_layouts("+-100", c, G, Q);
            // a whole row and a whole column at 100
            if (G >= 1) {
                for (float &x : c)
                    x = uni(rng);
                for (int q = 0; q < Q; ++q)
                    c[q] = 100.f;
                for (int g = 0; g < G; ++g)
                    c[(size_t)g * Q] = 100.f;
                all_layouts("row and column of 100", c, G, Q);
            }
            problems += 4;
        }
    }
    // a cost without a finite assignment is refused, not looped on
    {
        std::vector<float> c(6, NAN);
        int32_t mq[2], mg[3];
        double u[2], v[3];
        if (rac_lsap_host(c.data(), 3, 1, 2, 3, mq, mg, u, v, nullptr) != -2) {
            fprintf(stderr, "FAIL: an all-NaN cost was not refused\n");
            ++g_failed;
        }
    }
    printf("lsap_check: %d problems x 3 layouts, %d failures\n", problems, g_failed);
    return g_failed ? 1 : 0;
}
