"""What an item-similarity measure is and which build a job takes (csrc/fy_itemsim_plan.hpp: isim_measure, isim_route; host-only C++,
built here with g++ alone, and once more with -fsanitize=address,undefined).

isim_measure is compared field by field with the table of include/filmyou.h, written out below.  isim_route is fed plain values: a
base case that takes the symmetric build, and every clause of the condition flipped on its own.  Everything asserted is a closed
form of the INPUT; nothing is compared with another output of the functions."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filmyou-core_amd", "csrc")

COSINE, COOCCURRENCE, TANIMOTO, LOGLIKELIHOOD, CITY_BLOCK, EUCLIDEAN, PEARSON = range(7)
RATING, ONE, CENTRED = 0, 1, 2              # IsimWeight
A_NONE, A_RATERS, A_SUMSQ = 0, 1, 2         # IsimNorm
FIN_SURV = 512                              # k_isim_finish sorts this many entries of a row: K <= FIN_SURV / 2 takes the symmetric build

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "fy_itemsim_plan.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ls(line);
        std::string what, name;
        if (!(ls >> what >> name)) continue;
        if (what == "measure") {
            int s;
            ls >> s;
            const fy::IsimMeasure m = fy::isim_measure(s);
            const int instantiated = fy::isim_dispatch(s, [](auto M) { return (int)decltype(M)::value; });
            printf("{\"name\": \"%s\", \"weight\": %d, \"finishes\": %d, \"counts\": %d, \"a\": %d, \"inv_norm\": %d, \"kernel\": %d, \"sweep\": %d, \"dispatch\": %d}\n",
                   name.c_str(), m.weight, (int)m.finishes, (int)m.counts, m.a, (int)m.inv_norm, m.kernel, (int)m.sweep, instantiated);
        } else {
            fy::IsimRouteInput in{};
            long long K, world, has_thr, Ic, exact, positive, gram, min_items, pk;
            unsigned long long mem;
            double thr;
            ls >> in.similarity >> K >> world >> has_thr >> thr >> Ic >> exact >> positive >> mem >> gram >> min_items >> pk;
            if (!ls) { fprintf(stderr, "%s: a route has 12 fields\n", name.c_str()); return 2; }
            in.K = (int32_t)K; in.world = (int32_t)world; in.has_threshold = has_thr != 0; in.threshold = thr; in.Ic = (int32_t)Ic;
            in.ratings_fp16_exact = exact != 0; in.ratings_positive = positive != 0; in.total_mem = mem;
            in.isim_gram = (int)gram; in.isim_gram_min_items = (int)min_items; in.cooc_pk = (int)pk;
            const fy::IsimRoute r = fy::isim_route(in);
            printf("{\"name\": \"%s\", \"symmetric\": %d, \"packed\": %d}\n", name.c_str(), (int)r.symmetric, (int)r.packed);
        }
    }
    printf("{\"name\": \"fin_surv\", \"value\": %d}\n", fy::ISIM_PLAN_FIN_SURV);
    return 0;
}
'''

# include/filmyou.h, "constant / column transform w_ui / norm a_i / similarity":
#   weight: r_ui (cosine: divided by ||r_.i||, the only measure with inv_norm) / 1 / the centred c_ui;  a: - / n_i / sum r^2;
#   finishes: the similarity is not d itself;  counts: a finishing measure on w = 1;  kernel: itself where it finishes, else cosine's;
#   sweep: the symmetric build admits cosine and the four finishing measures
TABLE = {
    "cosine": (COSINE, dict(weight=RATING, finishes=0, counts=0, a=A_NONE, inv_norm=1, kernel=COSINE, sweep=1)),
    "cooccurrence": (COOCCURRENCE, dict(weight=ONE, finishes=0, counts=0, a=A_NONE, inv_norm=0, kernel=COSINE, sweep=0)),
    "tanimoto": (TANIMOTO, dict(weight=ONE, finishes=1, counts=1, a=A_RATERS, inv_norm=0, kernel=TANIMOTO, sweep=1)),
    "loglikelihood": (LOGLIKELIHOOD, dict(weight=ONE, finishes=1, counts=1, a=A_RATERS, inv_norm=0, kernel=LOGLIKELIHOOD, sweep=1)),
    "city_block": (CITY_BLOCK, dict(weight=ONE, finishes=1, counts=1, a=A_RATERS, inv_norm=0, kernel=CITY_BLOCK, sweep=1)),
    "euclidean": (EUCLIDEAN, dict(weight=RATING, finishes=1, counts=0, a=A_SUMSQ, inv_norm=0, kernel=EUCLIDEAN, sweep=1)),
    "pearson": (PEARSON, dict(weight=CENTRED, finishes=0, counts=0, a=A_NONE, inv_norm=0, kernel=COSINE, sweep=0)),
}

IC = 59047                                   # ML-25M's items
LDM = (IC + 255) // 256 * 256
MATRIX = IC * LDM * 4                        # bytes of the fp32 half Gram
# cosine at benchmark size on one rank with the defaults: the symmetric build
BASE = dict(similarity=COSINE, K=100, world=1, has_threshold=0, threshold=0.0, Ic=IC, exact=1, positive=1, mem=288 << 30, gram=-1, min_items=4096, pk=1)
ORDER = ["similarity", "K", "world", "has_threshold", "threshold", "Ic", "exact", "positive", "mem", "gram", "min_items", "pk"]

ROUTES = {"base": {}}


def route(name, **kw):
    ROUTES[name] = kw
    return name


# (case, symmetric, packed): one line per clause
EXPECT = [
    ("base", 1, 1),
    (route("world_2", world=2), 0, 1),
    (route("cooc_pk_0", pk=0), 0, 0),
    (route("not_fp16_exact", exact=0), 0, 0),
    (route("not_positive", positive=0), 0, 1),
    (route("euclidean_forced", similarity=EUCLIDEAN, gram=1), 1, 1),
    (route("euclidean_forced_not_fp16_exact", similarity=EUCLIDEAN, gram=1, exact=0), 0, 0),
    (route("tanimoto_forced", similarity=TANIMOTO, gram=1), 1, 1),
    # a count measure multiplies ones: exact whatever the ratings are
    (route("tanimoto_forced_not_fp16_exact", similarity=TANIMOTO, gram=1, exact=0), 1, 0),
    (route("tanimoto_forced_not_positive", similarity=TANIMOTO, gram=1, positive=0), 1, 1),
    (route("loglikelihood_forced_neither", similarity=LOGLIKELIHOOD, gram=1, exact=0, positive=0), 1, 0),
    (route("k_half_fin_surv", K=FIN_SURV // 2), 1, 1),
    (route("k_half_fin_surv_plus_1", K=FIN_SURV // 2 + 1), 0, 1),
    (route("threshold_positive", has_threshold=1, threshold=0.25), 1, 1),
    (route("threshold_zero", has_threshold=1, threshold=0.0), 0, 1),
    (route("threshold_negative", has_threshold=1, threshold=-0.5), 0, 1),
    (route("threshold_zero_not_set", has_threshold=0, threshold=0.0), 1, 1),
    (route("gram_0_cosine", gram=0), 0, 1),
    (route("gram_auto_cosine", gram=-1), 1, 1),
    (route("gram_1_cosine", gram=1), 1, 1),
    (route("gram_0_city_block", similarity=CITY_BLOCK, gram=0), 0, 1),
    (route("gram_auto_city_block", similarity=CITY_BLOCK, gram=-1), 0, 1),       # the other measures: forced only
    (route("gram_1_city_block", similarity=CITY_BLOCK, gram=1), 1, 1),
    (route("items_below_minimum", Ic=4095, mem=288 << 30), 0, 1),
    (route("items_at_minimum", Ic=4096), 1, 1),
    (route("items_below_minimum_forced", Ic=4095, gram=1), 1, 1),              # the minimum belongs to the automatic choice
    # Ic * round_up(Ic, 256) * 4 > total_mem / 3 refuses: total_mem / 3 (integer) == the matrix still fits, one byte less does not
    (route("memory_exactly_fits", mem=3 * MATRIX), 1, 1),
    (route("memory_fits_by_the_division", mem=3 * MATRIX + 2), 1, 1),
    (route("memory_one_short", mem=3 * MATRIX - 1), 0, 1),
    (route("pearson_auto", similarity=PEARSON), 0, 0),
    (route("pearson_forced", similarity=PEARSON, gram=1), 0, 0),                 # never symmetric, never packed
    (route("cooccurrence_auto", similarity=COOCCURRENCE), 0, 1),
    (route("cooccurrence_forced", similarity=COOCCURRENCE, gram=1), 0, 1),
    (route("cooccurrence_not_fp16_exact", similarity=COOCCURRENCE, exact=0), 0, 0),
]


def build_driver(d, *flags):
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = str(d / ("drv" + "".join(flags).replace("=", "_").replace(",", "_")))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", exe, str(src)], check=True)
    return exe


def run_driver(exe):
    lines = ["measure %s %d" % (name, s) for name, (s, _) in TABLE.items()]
    for name, kw in ROUTES.items():
        v = dict(BASE, **kw)
        lines.append("route %s %s" % (name, " ".join(repr(v[k]) for k in ORDER)))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = [json.loads(line) for line in r.stdout.splitlines()]
    assert [g["name"] for g in got] == list(TABLE) + list(ROUTES) + ["fin_surv"]
    return {g["name"]: g for g in got}


@pytest.fixture(scope="module")
def driver_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("itemsim_plan")


@pytest.fixture(scope="module")
def planned(driver_dir):
    return run_driver(build_driver(driver_dir))


@pytest.mark.parametrize("name", list(TABLE))
def test_measure_is_the_row_of_the_table(planned, name):
    s, want = TABLE[name]
    got = planned[name]
    assert {k: got[k] for k in want} == want
    assert got["dispatch"] == want["kernel"]      # the one switch on the launch side instantiates what the table names


def test_the_cases_flip_one_clause_each():
    assert len(ROUTES) == len(EXPECT) and len({e[0] for e in EXPECT}) == len(EXPECT)
    assert MATRIX == 59047 * 59136 * 4 and (3 * MATRIX + 2) // 3 == MATRIX and (3 * MATRIX - 1) // 3 == MATRIX - 1


@pytest.mark.parametrize("name,symmetric,packed", EXPECT, ids=[e[0] for e in EXPECT])
def test_route(planned, name, symmetric, packed):
    assert (planned[name]["symmetric"], planned[name]["packed"]) == (symmetric, packed)


def test_the_header_states_the_finish_kernels_limit(planned):
    assert planned["fin_surv"]["value"] == FIN_SURV


def test_same_answers_under_address_and_undefined_behaviour_sanitizers(driver_dir, planned):
    """a stand-alone program: the sanitizers' runtimes are linked in, nothing is preloaded"""
    got = run_driver(build_driver(driver_dir, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert got == planned
