// fy_partition.hpp -- which rank owns which clusters (host only: no HIP include, compiled by g++ in tests/test_partition_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fy {

// Cuts `w` (one weight per position, in order) into `parts` contiguous runs with the smallest possible largest run (binary search on the
// cap, greedy fill), and -- when there are at least as many positions as parts -- leaves NO run empty: the greedy fill may need fewer
// runs than parts ([10, 1, 1] on 3: cap 10, runs [10] [1, 1]); runs of two or more positions are then cut (the heaviest first, at its most
// even cut) until there are `parts` of them, which never raises the largest run.  Returns the first position of every run (parts + 1
// entries); only with fewer positions than parts are the trailing runs empty.
inline std::vector<int> linear_partition(const std::vector<int64_t>& w, int parts) {
    const int n = (int)w.size();
    auto runs_needed = [&](int64_t cap, std::vector<int>* first) -> int {
        int runs = 1;
        int64_t in_run = 0;
        if (first) { first->clear(); first->push_back(0); }
        for (int k = 0; k < n; k++) {
            if (w[(size_t)k] > cap) return parts + 1;
            if (in_run + w[(size_t)k] > cap && in_run > 0) { runs++; in_run = 0; if (first) first->push_back(k); }
            in_run += w[(size_t)k];
        }
        return runs;
    };
    int64_t lo = 0, hi = 0;
    for (int64_t x : w) hi += x;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (runs_needed(mid, nullptr) <= parts) hi = mid; else lo = mid + 1;
    }
    std::vector<int> first;
    runs_needed(hi, &first);
    first.push_back(n);         // first[r] .. first[r + 1]: run r
    while ((int)first.size() < parts + 1 && (int)first.size() - 1 < n) {
        int best = -1;
        int64_t best_w = -1;
        for (int r = 0; r + 1 < (int)first.size(); r++) {
            if (first[(size_t)r + 1] - first[(size_t)r] < 2) continue;
            int64_t s = 0;
            for (int k = first[(size_t)r]; k < first[(size_t)r + 1]; k++) s += w[(size_t)k];
            if (s > best_w) { best_w = s; best = r; }
        }
        // (fewer runs than positions: some run holds two)
        const int a = first[(size_t)best], b = first[(size_t)best + 1];
        int cut = a + 1;
        int64_t left = 0, best_max = -1;
        for (int k = a + 1; k < b; k++) {
            left += w[(size_t)k - 1];
            const int64_t m = left > best_w - left ? left : best_w - left;
            if (best_max < 0 || m < best_max) { best_max = m; cut = k; }
        }
        first.insert(first.begin() + best + 1, cut);
    }
    while ((int)first.size() < parts + 1) first.push_back(n);
    return first;
}

}  // namespace fy
