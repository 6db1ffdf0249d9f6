// lsap_host.cpp -- rectangular linear sum assignment on the host, plain C++ (no HIP): the solver behind the CPU route of the
// assigners (racformer_amd/losses.py), behind RaCFormer_head.loss_unfused and behind any problem with more ground-truth boxes
// than queries.  Same algorithm and arithmetic as rac_lsap_fwd (match.hip): shortest augmenting paths with dual variables
// (Jonker-Volgenant as restated by Crouse, "On implementing 2D rectangular assignment algorithms", IEEE TAES 2016 -- what
// scipy.optimize.linear_sum_assignment implements), float64 throughout, the float32 cost widened on read.  Ties of the
// per-step minimum go to the smaller index.
#include <stdint.h>
#include <limits>
#include <vector>
#include "../../include/racformer_hip.h"

void rac_set_error(const char *fmt, ...);

namespace {

// rows: the side that is iterated (nr <= nc), columns: the scanned side.  at(i, j): cost of row i / column j.
// col4row [nr], row4col [nc], u [nr], v [nc].  Returns the number of Dijkstra steps, or -1 if a row found no finite path.
template <typename At>
long solve(int nr, int nc, At at, std::vector<int> &col4row, std::vector<int> &row4col, std::vector<double> &u,
           std::vector<double> &v)
{
    const double inf = std::numeric_limits<double>::infinity();
    col4row.assign(nr, -1);
    row4col.assign(nc, -1);
    u.assign(nr, 0.0);
    v.assign(nc, 0.0);
    std::vector<double> shortest(nc);
    std::vector<int> path(nc);
    std::vector<char> scanned(nc);
    std::vector<int> scanned_list;
    long steps = 0;
    for (int cur = 0; cur < nr; ++cur) {
        std::fill(shortest.begin(), shortest.end(), inf);
        std::fill(scanned.begin(), scanned.end(), 0);
        scanned_list.clear();
        double min_val = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            int index = -1;
            double lowest = inf;
            const double ui = u[i];
            for (int j = 0; j < nc; ++j) {
                if (scanned[j])
                    continue;
                const double r = min_val + (double)at(i, j) - ui - v[j];
                if (r < shortest[j]) {
                    shortest[j] = r;
                    path[j] = i;
                }
                if (shortest[j] < lowest) {
                    lowest = shortest[j];
                    index = j;
                }
            }
            ++steps;
            if (index < 0)
                return -1;      // (no finite entry left: NaN or +inf costs)
            min_val = lowest;
            scanned[index] = 1;
            scanned_list.push_back(index);
            if (row4col[index] < 0)
                sink = index;
            else
                i = row4col[index];
        }
        // duals: the rows reached are cur and the rows of the scanned, assigned columns
        u[cur] += min_val;
        for (int j : scanned_list) {
            const double d = min_val - shortest[j];
            if (j != sink)
                u[row4col[j]] += d;
            v[j] -= d;
        }
        // augment along the path back to cur
        int j = sink;
        for (;;) {
            const int r = path[j];
            row4col[j] = r;
            const int prev = col4row[r];
            col4row[r] = j;
            j = prev;
            if (r == cur)
                break;
        }
    }
    return steps;
}

}   // namespace

extern "C" int rac_lsap_host(const float *cost, int64_t gt_stride, int64_t query_stride, int num_gt, int num_query,
                             int32_t *matched_query, int32_t *matched_gt, double *u, double *v, int64_t *steps)
{
    if (num_gt < 0 || num_query < 0) {
        rac_set_error("rac_lsap_host: num_gt=%d num_query=%d", num_gt, num_query);
        return RAC_E_ARG;
    }
    if ((num_gt > 0 && (!matched_query || !u)) || (num_query > 0 && (!matched_gt || !v)) || (num_gt > 0 && num_query > 0 && !cost)) {
        rac_set_error("rac_lsap_host: null pointer");
        return RAC_E_ARG;
    }
    std::vector<int> col4row, row4col;
    std::vector<double> du, dv;
    long n;
    const bool by_gt = num_gt <= num_query;     // iterate over the smaller side
    if (by_gt)
        n = solve(num_gt, num_query, [&](int g, int q) { return cost[g * gt_stride + q * query_stride]; }, col4row, row4col, du, dv);
    else
        n = solve(num_query, num_gt, [&](int q, int g) { return cost[g * gt_stride + q * query_stride]; }, col4row, row4col, du, dv);
    if (n < 0) {
        rac_set_error("rac_lsap_host: the cost matrix has no finite assignment (NaN or infinite entries)");
        return RAC_E_UNSUPPORTED;
    }
    const std::vector<int> &q_of_g = by_gt ? col4row : row4col, &g_of_q = by_gt ? row4col : col4row;
    const std::vector<double> &ug = by_gt ? du : dv, &vq = by_gt ? dv : du;
    for (int g = 0; g < num_gt; ++g) {
        matched_query[g] = q_of_g[g];
        u[g] = ug[g];
    }
    for (int q = 0; q < num_query; ++q) {
        matched_gt[q] = g_of_q[q];
        v[q] = vq[q];
    }
    if (steps)
        *steps = n;
    return 0;
}
