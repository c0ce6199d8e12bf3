"""Which rank owns which clusters (csrc/fy_partition.hpp, host-only C++, built here with g++): contiguous runs over the non-empty
clusters in ascending id, the largest run as small as it can be, and -- with at least as many clusters as ranks -- NO rank without a
cluster.  Checked against an exhaustive optimum computed in this file.

The case that started it: weights [10, 1, 1] on 3 ranks.  The min-cap greedy alone needs two runs ([10] [1, 1]); padded to three, the
third rank owned nothing although three non-empty clusters exist (first = [0, 1, 3, 3])."""
import functools
import itertools
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filmyou-core_amd", "csrc")

DRIVER = r'''
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "fy_partition.hpp"
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int parts;
        in >> parts;
        std::vector<int64_t> w;
        long long x;
        while (in >> x) w.push_back((int64_t)x);
        const std::vector<int> first = fy::linear_partition(w, parts);
        for (size_t k = 0; k < first.size(); k++) printf(k ? " %d" : "%d", first[k]);
        printf("\n");
    }
    return 0;
}
'''


@functools.lru_cache(maxsize=None)
def optimum(w, parts):
    """smallest possible largest run over EVERY way to cut the tuple w into `parts` non-empty contiguous runs (all first cuts tried,
    the rest by recursion; memoised on the suffix)"""
    if parts == 1:
        return sum(w)
    return min(max(sum(w[:c]), optimum(w[c:], parts - 1)) for c in range(1, len(w) - parts + 2))


def cases():
    out = [((10, 1, 1), 3)]
    for n in range(1, 8):
        for w in itertools.product((1, 2, 5, 40), repeat=n):
            for parts in range(1, n + 1):
                out.append((w, parts))
    rng = random.Random(20)
    for _ in range(400):
        n = rng.randint(8, 60)
        kind = rng.randrange(3)
        if kind == 0:
            w = [rng.randint(1, 50) for _ in range(n)]
        elif kind == 1:                                   # one cluster far heavier than the rest, anywhere
            w = [rng.randint(1, 5) for _ in range(n)]
            w[rng.randrange(n)] = rng.randint(100, 100000)
        else:                                             # the library's weights: ~1e9 and more per cluster
            w = [rng.randint(1, 1 << 40) for _ in range(n)]
        out.append((tuple(w), rng.randint(1, min(n, 16))))
    return out


def test_linear_partition_against_the_exhaustive_optimum(tmp_path):
    src = tmp_path / "drv.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "drv")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(src)], check=True)
    todo = cases()
    text = "".join("%d %s\n" % (parts, " ".join(map(str, w))) for w, parts in todo)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(todo)
    for (w, parts), line in zip(todo, lines):
        first = [int(x) for x in line.split()]
        where = (w, parts, first)
        assert len(first) == parts + 1 and first[0] == 0 and first[-1] == len(w), where      # contiguous, everything covered
        assert all(a < b for a, b in zip(first, first[1:])), where                           # length >= parts: no run is empty
        largest = max(sum(w[a:b]) for a, b in zip(first, first[1:]))
        assert largest == optimum(w, parts), where + (largest, optimum(w, parts))


def test_fewer_positions_than_parts_pads_with_empty_runs(tmp_path):
    """(the library never asks for it -- it shards only with at least as many non-empty clusters as ranks -- but the function answers:
    every position a run of its own, the trailing runs empty)"""
    src = tmp_path / "drv.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "drv")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(src)], check=True)
    r = subprocess.run([exe], input="4 7 3\n3\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == ["0 1 2 2 2", "0 0 0 0"]
