"""How an RM2 job scores its clusters (csrc/fy_rm2_plan.hpp: plan_job, host-only C++, built here with g++): packed or fp32 rows, pruned
or full pass, cooperative, column panel, symmetric panel, flat batch, panel groups, lanes, batch and buffer sizes.

Every field of every Plan and of the JobPlan is compared with tests/golden/rm2_plans.json.  The golden values were NOT produced by
fy_rm2_plan.hpp: they come from the planning lines of fy::rm2_score as they stood inline in fy_rm2.hip before the split, compiled
verbatim behind stubbed inputs (same text protocol as the driver below), so the file pins the behaviour the split had to keep.  The
invariants the scoring flows rely on are asserted on top of it, whatever the golden says.

A forced cooc_max_ch too small for 255 chunks per row: the first pick widens such a width to ceil(Ic / 255) columns rounded up to
256, so it never fails (forced_cooc_max_ch_64 records the widened plan).  Panel mode picks the chunks again, capped by the forced
width, and the inline planning did not look at the count after that: 50 clusters of 30 000 items with cooc_max_ch = 64 were planned
with 469 chunks of 64 columns, which the row kernel's 8-bit chunk ids cannot hold.  plan_job refuses that plan with the error the
first pick has.  That case (NOT_FROM_PARENT) is therefore the one whose expected value is stated here and not in the golden file."""
import json
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filmyou-core_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rm2_plans.json")

# ---------------------------------------------------------------- text protocol (shared with the harness that wrote the golden file)
# One case per line, `key=value` tokens; vectors are comma separated.  The reader fills a CaseInput, the writer prints one JSON
# object per case from anything that has JobPlan's members.
DRIVER_IO = r'''
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct CaseInput {
    std::string name;
    int32_t K = 0, nU = 0;
    std::vector<int32_t> csize, ucstart, pcstart, cluster_q, work_lo, work_hi;     // work_*: the work-balanced slot range of every rank
    std::vector<int64_t> cluster_deg2;
    int64_t sum_deg2 = 0;
    bool fp16 = true;
    std::vector<float> fx;
    int32_t N = 0, rank = 0, world = 1;
    double lambda = 0.5;
    int64_t workspace_bytes = 0, n_recs = 0;
    uint64_t total_mem = 0;
    bool sharded = false, have_coll = false;
    fy::Tuning tune;
};

template <class T>
static std::vector<T> parse_list(const std::string& v) {
    std::vector<T> out;
    std::stringstream ss(v);
    std::string tok;
    while (std::getline(ss, tok, ','))
        if (!tok.empty()) out.push_back((T)std::strtod(tok.c_str(), nullptr));      // (strtod reads "nan" and "inf" too)
    return out;
}

static bool parse_case(const std::string& line, CaseInput& in) {
    std::istringstream ls(line);
    std::string tok;
    bool any = false;
    while (ls >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); exit(2); }
        const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
        any = true;
        fy::Tuning& t = in.tune;
#define KNOB(name) else if (k == "tune." #name) t.name = (decltype(t.name))std::strtod(v.c_str(), nullptr)
        if (k == "name") in.name = v;
        else if (k == "K") in.K = atoi(v.c_str());
        else if (k == "nU") in.nU = atoi(v.c_str());
        else if (k == "csize") in.csize = parse_list<int32_t>(v);
        else if (k == "ucstart") in.ucstart = parse_list<int32_t>(v);
        else if (k == "pcstart") in.pcstart = parse_list<int32_t>(v);
        else if (k == "cluster_q") in.cluster_q = parse_list<int32_t>(v);
        else if (k == "work_lo") in.work_lo = parse_list<int32_t>(v);
        else if (k == "work_hi") in.work_hi = parse_list<int32_t>(v);
        else if (k == "cluster_deg2") in.cluster_deg2 = parse_list<int64_t>(v);
        else if (k == "sum_deg2") in.sum_deg2 = atoll(v.c_str());
        else if (k == "fp16") in.fp16 = atoi(v.c_str()) != 0;
        else if (k == "fx") in.fx = parse_list<float>(v);
        else if (k == "N") in.N = atoi(v.c_str());
        else if (k == "rank") in.rank = atoi(v.c_str());
        else if (k == "world") in.world = atoi(v.c_str());
        else if (k == "lambda") in.lambda = atof(v.c_str());
        else if (k == "workspace_bytes") in.workspace_bytes = atoll(v.c_str());
        else if (k == "n_recs") in.n_recs = atoll(v.c_str());
        else if (k == "total_mem") in.total_mem = strtoull(v.c_str(), nullptr, 10);
        else if (k == "sharded") in.sharded = atoi(v.c_str()) != 0;
        else if (k == "have_coll") in.have_coll = atoi(v.c_str()) != 0;
        KNOB(seed_chunks); KNOB(seed_forced); KNOB(lanes); KNOB(lanes_forced); KNOB(panel_sym); KNOB(panel_two_phase); KNOB(panel_multi_launch);
        KNOB(flat_batch); KNOB(prune); KNOB(pack24); KNOB(cooc_pk); KNOB(coop); KNOB(coop_force); KNOB(cooc_max_ch); KNOB(flat_budget);
        KNOB(panel_group_bytes); KNOB(pack24_min_items); KNOB(prune_min_items); KNOB(prune_min_users); KNOB(panel_min_clusters); KNOB(panel_cols);
        KNOB(panel_wide_below_users); KNOB(panel_max_ch); KNOB(panel_lanes); KNOB(cooc_half); KNOB(cooc_fx); KNOB(cooc_f32); KNOB(full_walk_sparse);
        KNOB(workspace_default);
        else { fprintf(stderr, "unknown key %s\n", k.c_str()); exit(2); }
#undef KNOB
    }
    return any;
}

static void print_error(const std::string& name, int code, const std::string& msg) {
    printf("{\"name\": \"%s\", \"error\": %d, \"msg\": \"%s\"}\n", name.c_str(), code, msg.c_str());
}

template <class JP>
static void print_plan(const std::string& name, const JP& j) {
    printf("{\"name\": \"%s\", \"error\": 0, \"use_pk\": %d, \"long_seed\": %d, \"short_seed_ok\": %d, \"seed_chunks\": %d, \"count_balanced\": %d, "
           "\"max_Ic\": %lld, \"eff_top\": %d, \"ws\": %lld, \"flat_budget\": %lld, \"any_panel\": %d, \"two_phase\": %d, \"n_groups\": %d, \"NS\": %d, "
           "\"any_coop\": %d, \"any_tail\": %d, \"any_half\": %d, \"co_all\": %llu, ",
           name.c_str(), (int)j.use_pk, (int)j.long_seed, (int)j.short_seed_ok, (int)j.seed_chunks, (int)j.count_balanced, (long long)j.max_Ic, (int)j.eff_top,
           (long long)j.ws, (long long)j.flat_budget, (int)j.any_panel, (int)j.two_phase, (int)j.n_groups, (int)j.NS, (int)j.any_coop, (int)j.any_tail,
           (int)j.any_half, (unsigned long long)j.co_all);
    printf("\"m_el\": %llu, \"s_el\": %llu, \"ov_el\": %llu, \"bm_el\": %llu, \"ub_el\": %llu, \"am_el\": %llu, \"gp_el\": %llu, \"b64_el\": %llu, \"a64_el\": %llu, "
           "\"is_el\": %llu, ",
           (unsigned long long)j.m_el, (unsigned long long)j.s_el, (unsigned long long)j.ov_el, (unsigned long long)j.bm_el, (unsigned long long)j.ub_el,
           (unsigned long long)j.am_el, (unsigned long long)j.gp_el, (unsigned long long)j.b64_el, (unsigned long long)j.a64_el, (unsigned long long)j.is_el);
    printf("\"h_gscale\": [");
    for (size_t k = 0; k < j.h_gscale.size(); k++) printf(k ? ", %.9g" : "%.9g", (double)j.h_gscale[k]);
    printf("], \"h_cshift\": [");
    for (size_t k = 0; k < j.h_cshift.size(); k++) printf(k ? ", %d" : "%d", (int)j.h_cshift[k]);
    printf("], \"group_of\": [");
    for (size_t k = 0; k < j.group_of.size(); k++) printf(k ? ", %d" : "%d", (int)j.group_of[k]);
    printf("], \"plans\": [");
    for (size_t k = 0; k < j.plans.size(); k++) {
        const auto& p = j.plans[k];
        printf("%s{\"c\": %d, \"Uc\": %d, \"sbase\": %d, \"pbase\": %d, \"Ic\": %d, \"a\": %d, \"b\": %d, \"CH\": %d, \"nch\": %d, \"q0\": %d, \"nq\": %d, \"ldm\": %lld, "
               "\"B\": %lld, \"pack24\": %d, \"prune\": %d, \"coop\": %d, \"half\": %d, \"panel\": %d, \"psym\": %d, \"flat\": %d, \"panel_cols\": %d, \"nsub\": %d, "
               "\"ldb64\": %lld, \"tail_chunks\": %d, \"p_eff\": %d, \"tail_width\": %d, \"nblk\": %d, \"ldb\": %lld}",
               k ? ", " : "", p.c, p.Uc, p.sbase, p.pbase, p.Ic, p.a, p.b, p.CH, p.nch, p.q0, p.nq, (long long)p.ldm, (long long)p.B, (int)p.pack24, (int)p.prune,
               (int)p.coop, (int)p.half, (int)p.panel, (int)p.psym, (int)p.flat, p.panel_cols, p.nsub, (long long)p.ldb64, p.tail_chunks, p.p_eff, p.tail_width,
               p.nblk, (long long)p.ldb);
    }
    printf("]}\n");
}
'''

DRIVER = r'''
#include "fy_rm2_plan.hpp"
''' + DRIVER_IO + r'''
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        CaseInput c;
        if (!parse_case(line, c)) continue;
        fy::PlanInput in;
        in.K = c.K; in.nU = c.nU;
        in.csize = c.csize; in.ucstart = c.ucstart; in.pcstart = c.pcstart; in.cluster_q = c.cluster_q;
        in.cluster_deg2 = c.cluster_deg2; in.sum_deg2 = c.sum_deg2;
        in.ratings_fp16_exact = c.fp16;
        in.fx_bounds = c.fx;
        in.number_of_recommendations = c.N; in.rank = c.rank; in.world = c.world;
        in.lambda = c.lambda;
        in.workspace_bytes = c.workspace_bytes;
        in.tune = c.tune;
        in.total_mem = c.total_mem;
        in.sharded = c.sharded; in.have_coll = c.have_coll;
        in.n_recs = c.n_recs;
        // every rank's owner range, as the job takes it AFTER the count-balanced decision: a sharded rank owns all users of its own
        // structure, count-balanced ranks equal counts, everybody else the work-balanced range
        const bool cb = fy::plan_count_balanced(in);
        for (int k = 0; k < c.world; k++) {
            int32_t lo = c.work_lo[(size_t)k], hi = c.work_hi[(size_t)k];
            if (c.sharded) { lo = 0; hi = k == c.rank ? c.nU : 0; }
            else if (cb) { lo = (int32_t)((int64_t)c.nU * k / c.world); hi = (int32_t)((int64_t)c.nU * (k + 1) / c.world); }
            in.own_lo.push_back(lo);
            in.own_hi.push_back(hi);
        }
        try {
            const fy::JobPlan jp = fy::plan_job(in);
            if (jp.count_balanced != cb) { fprintf(stderr, "%s: plan_job and plan_count_balanced disagree\n", c.name.c_str()); return 3; }
            print_plan(c.name, jp);
        } catch (const fy::PlanError& e) {
            print_error(c.name, e.code, e.msg);
        }
    }
    return 0;
}
'''

NOT_FROM_PARENT = {"error_forced_cooc_max_ch_64_panel_mode"}      # (see the docstring; the harness that writes the golden file leaves it out)

HBM = 288 << 30      # bytes of HBM the plans are made for


def case(name, Uc, Ic, N, deg2=None, fx=(40.0, 0.05, 5.0), world=1, rank=0, work=None, n_recs=None, tune=None, sharded=0, have_coll=0, lam=0.5,
         ws=0, total_mem=HBM, fp16=1, ratings_per_user=100):
    """Uc / Ic: one number per cluster.  fx: one triple for every cluster, or a flat list (possibly short, possibly empty).
    work: the work-balanced slot range of every rank (default: rank 0 owns everything)."""
    K = len(Uc)
    assert len(Ic) == K
    ucstart = [0]
    pcstart = [0]
    cluster_q = [0]
    for u, i in zip(Uc, Ic):
        ucstart.append(ucstart[-1] + u)
        pcstart.append(pcstart[-1] + i)
        cluster_q.append(cluster_q[-1] + u * ratings_per_user)
    nU = ucstart[-1]
    if deg2 is None:
        deg2 = [3 * u * ratings_per_user * ratings_per_user for u in Uc]
    if work is None:
        work = [(0, nU)] + [(nU, nU)] * (world - 1)
    assert len(work) == world
    if isinstance(fx, tuple):
        fx = list(fx) * K
    if n_recs is None:      # every user of this rank's work range gets min(N, Ic) entries
        lo, hi = work[rank] if not sharded else (0, nU)
        n_recs = sum(max(0, min(hi, ucstart[c + 1]) - max(lo, ucstart[c])) * min(N, Ic[c]) for c in range(K))
    f = lambda xs: ",".join(str(x) for x in xs)
    toks = ["name=" + name, "K=%d" % K, "nU=%d" % nU, "csize=" + f(Uc), "ucstart=" + f(ucstart), "pcstart=" + f(pcstart), "cluster_q=" + f(cluster_q),
            "cluster_deg2=" + f(deg2), "sum_deg2=%d" % sum(deg2), "fp16=%d" % fp16, "N=%d" % N, "rank=%d" % rank, "world=%d" % world,
            "lambda=%r" % lam, "workspace_bytes=%d" % ws, "n_recs=%d" % n_recs, "total_mem=%d" % total_mem, "sharded=%d" % sharded,
            "have_coll=%d" % have_coll, "work_lo=" + f(w[0] for w in work), "work_hi=" + f(w[1] for w in work)]
    if fx:
        toks.append("fx=" + f(fx))
    for k, v in (tune or {}).items():
        toks.append("tune.%s=%s" % (k, v))
    return " ".join(toks)


def cases():
    out = []
    # one cluster (ML-25M shape)
    out.append(case("one_cluster_N100", [162541], [59047], 100))
    out.append(case("one_cluster_N1000", [162541], [59047], 1000))
    # 50 clusters: panel mode, two phases, symmetric panels
    out.append(case("c50_N100", [3250] * 50, [30000] * 50, 100))
    # ... long lists: the full pass; cluster_deg2 below and above Ic^2 in turn (full_walk_sparse)
    out.append(case("c50_N1000_deg2_both_sides", [3250] * 50, [30000] * 50, 1000, deg2=[30000 * 30000 - 1 if c % 2 == 0 else 30000 * 30000 + 1 for c in range(50)]))
    # the panel is no multiple of the chunk: re-pick / widen
    out.append(case("c50_netflix_shape", [9600] * 50, [17770] * 50, 100))
    # doubled panel for clusters under 2500 users; three panel groups
    out.append(case("c200_N100", [812] * 200, [20000] * 200, 100))
    out.append(case("c200_three_groups", [812] * 200, [20000] * 200, 100, tune={"panel_group_bytes": 38500000000}))
    # flat batches
    out.append(case("c400_flat", [406] * 400, [9000] * 400, 100))
    out.append(case("c400_flat_budget_excludes_some", [406] * 400, [12000 if c % 10 == 0 else 9000 for c in range(400)], 100, tune={"flat_budget": 300000000}))
    out.append(case("c400_fewer_than_two_flat", [406] * 400, [4200 if c == 7 else 9000 for c in range(400)], 100, tune={"flat_budget": 100000000}))
    # mixed: three prunable clusters (fewer than panel_min_clusters) beside small ones that keep fp32 rows
    out.append(case("mixed_prunable_and_fp32", [5000, 300, 5000, 200, 5000, 100, 50, 700], [20000, 3000, 20000, 2500, 20000, 1000, 900, 4000], 100))
    # two ranks with collectives
    for r in (0, 1):
        out.append(case("two_ranks_count_balanced_r%d" % r, [0, 162541, 0], [0, 59047, 0], 100, world=2, rank=r, have_coll=1,
                        work=[(0, 40000), (40000, 162541)]))
        out.append(case("two_ranks_coop_and_not_r%d" % r, [20000, 8000, 8000], [20000, 20000, 20000], 100, world=2, rank=r, have_coll=1,
                        work=[(0, 15000), (15000, 36000)]))
    out.append(case("two_ranks_no_collectives_r1", [20000, 8000, 8000], [20000, 20000, 20000], 100, world=2, rank=1, have_coll=0,
                    work=[(0, 15000), (15000, 36000)]))
    # sharded prep
    out.append(case("sharded_rank_without_users", [0, 0, 0], [0, 0, 0], 100, world=2, rank=1, sharded=1, have_coll=1, work=[(0, 0), (0, 0)]))
    out.append(case("sharded_rank_with_two_clusters", [0, 9000, 0, 7000], [0, 21000, 0, 18000], 100, world=2, rank=0, sharded=1, have_coll=1,
                    work=[(0, 0), (0, 0)]))
    # fx_bounds: fine, zero, NaN, infinite, a shift above 64, missing (the vector ends after five clusters)
    out.append(case("fx_bounds_kinds", [1000] * 6, [8192] * 6, 100,
                    fx=[40.0, 0.05, 5.0, 0.0, 0.0, 5.0, "nan", 0.05, 5.0, "inf", 0.05, 5.0, 1e20, 0.05, 5.0]))
    out.append(case("fx_bounds_none", [1000] * 6, [8192] * 6, 100, fx=[]))
    out.append(case("fx_bounds_none_one_cluster", [162541], [59047], 100, fx=[]))
    # knobs away from their defaults
    out.append(case("knob_seed_forced", [3250] * 50, [30000] * 50, 1000, tune={"seed_chunks": 3, "seed_forced": 1}))
    out.append(case("knob_lanes_forced", [3250] * 50, [30000] * 50, 100, tune={"lanes": 3, "lanes_forced": 1}))
    out.append(case("knob_panel_sym_0", [9600] * 50, [17770] * 50, 100, tune={"panel_sym": 0}))
    out.append(case("knob_panel_two_phase_0", [3250] * 50, [30000] * 50, 100, tune={"panel_two_phase": 0}))
    out.append(case("knob_panel_multi_launch_0", [3250] * 50, [30000] * 50, 100, tune={"panel_multi_launch": 0}))
    out.append(case("knob_flat_batch_0", [406] * 40, [9000] * 40, 100, tune={"flat_batch": 0}))
    out.append(case("knob_prune_0", [162541], [59047], 100, tune={"prune": 0}))
    out.append(case("knob_prune_0_c50", [3250] * 50, [30000] * 50, 100, tune={"prune": 0}))
    out.append(case("knob_pack24_0", [162541], [59047], 100, tune={"pack24": 0}))
    out.append(case("knob_cooc_pk_0", [162541], [59047], 100, tune={"cooc_pk": 0}))
    out.append(case("knob_cooc_pk_0_c50", [3250] * 50, [30000] * 50, 100, tune={"cooc_pk": 0}))
    out.append(case("knob_coop_force", [162541], [59047], 100, tune={"coop_force": 1}))
    out.append(case("ratings_not_fp16_exact_c40", [406] * 40, [9000] * 40, 100, fp16=0))
    out.append(case("small_workspace", [162541], [59047], 1000, ws=1 << 30))
    out.append(case("no_lists_asked_for", [162541], [59047], 0))
    # the error cases (the first is none: see the module's docstring)
    out.append(case("forced_cooc_max_ch_64", [162541], [59047], 100, tune={"cooc_max_ch": 64}))
    out.append(case("error_forced_cooc_max_ch_64_panel_mode", [3250] * 50, [30000] * 50, 100, tune={"cooc_max_ch": 64}))
    out.append(case("error_list_longer_than_topn_max", [162541], [59047], 3000))
    out.append(case("error_count_balanced_without_pruned_cluster", [500], [59047], 100, world=2, rank=0, have_coll=1, work=[(0, 100), (100, 500)]))
    return out


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    d = tmp_path_factory.mktemp("rm2_plan")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = str(d / "drv")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(src)], check=True)
    r = subprocess.run([exe], input="\n".join(cases()) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(got) == len(cases())
    return {g["name"]: g for g in got}


@pytest.fixture(scope="module")
def golden():
    """(the file keeps the plans of a case column by column, and every regular list as an arithmetic progression or as runs of
    equal values: lossless, and a fiftieth of the size)"""
    def dec(v):
        if isinstance(v, dict) and "runs" in v:
            return [x for x, n in v["runs"] for _ in range(n)]
        if isinstance(v, dict):
            return [v["from"] + k * v["step"] for k in range(v["n"])]
        return v

    with open(GOLDEN) as f:
        cases_ = json.load(f)
    for g in cases_:
        if "plans" in g:
            cols = {k: dec(v) for k, v in g["plans"]["columns"].items()}
            g["plans"] = [{k: cols[k][r] for k in cols} for r in range(g["plans"]["n"])]
        for k in ("h_gscale", "h_cshift", "group_of"):
            if k in g:
                g[k] = dec(g[k])
    return {g["name"]: g for g in cases_}


def test_every_field_of_every_plan_matches_the_inline_planning_it_was_split_from(planned, golden):
    assert sorted(set(planned) - NOT_FROM_PARENT) == sorted(golden)
    for name, want in golden.items():
        got = planned[name]
        assert sorted(got) == sorted(want), name
        for key in want:
            if key == "plans":
                assert len(got["plans"]) == len(want["plans"]), name
                for k, (pg, pw) in enumerate(zip(got["plans"], want["plans"])):
                    assert pg == pw, (name, "plan %d" % k, {f: (pg.get(f), pw[f]) for f in pw if pg.get(f) != pw[f]})
            else:
                assert got[key] == want[key], (name, key, got[key], want[key])


def test_the_cases_take_the_branches_they_are_named_for(planned):
    P = planned
    one = P["one_cluster_N100"]
    assert one["NS"] == 1 and len(one["plans"]) == 1 and one["plans"][0]["prune"] and one["plans"][0]["half"] and not one["plans"][0]["panel"]
    assert P["one_cluster_N1000"]["long_seed"] and P["one_cluster_N1000"]["plans"][0]["prune"]
    c50 = P["c50_N100"]
    assert c50["two_phase"] and c50["any_panel"] and all(p["panel"] and p["psym"] for p in c50["plans"]) and c50["NS"] == 8
    long50 = P["c50_N1000_deg2_both_sides"]
    assert not any(p["prune"] for p in long50["plans"])
    assert [p["half"] for p in long50["plans"]] == [c % 2 == 1 for c in range(50)]      # deg2 < Ic^2: full rows, no mirror
    nf = P["c50_netflix_shape"]["plans"][0]
    assert nf["panel"] and nf["panel_cols"] % nf["CH"] == 0 and nf["panel_cols"] != 4096      # widened or re-picked, not the knob's width
    assert P["c200_N100"]["plans"][0]["panel_cols"] == 8192 and P["c200_N100"]["n_groups"] == 2      # 113 GB of panels, a third of the HBM per group
    assert P["c200_three_groups"]["n_groups"] == 3
    assert all(p["flat"] for p in P["c400_flat"]["plans"])
    some = [p["flat"] for p in P["c400_flat_budget_excludes_some"]["plans"]]
    assert some == [c % 10 != 0 for c in range(400)]
    assert not any(p["flat"] for p in P["c400_fewer_than_two_flat"]["plans"])
    mixed = P["mixed_prunable_and_fp32"]
    assert sum(p["prune"] for p in mixed["plans"]) == 3 and not mixed["any_panel"] and any(not p["pack24"] for p in mixed["plans"])
    for r in (0, 1):
        cb = P["two_ranks_count_balanced_r%d" % r]
        assert cb["count_balanced"] and cb["plans"][0]["coop"] and cb["plans"][0]["b"] - cb["plans"][0]["a"] in (81270, 81271)
    assert [p["coop"] for p in P["two_ranks_coop_and_not_r1"]["plans"]] == [True, False, False]
    assert [p["coop"] for p in P["two_ranks_coop_and_not_r0"]["plans"]] == [True]
    assert not P["two_ranks_no_collectives_r1"]["any_coop"]
    assert P["sharded_rank_without_users"]["plans"] == [] and len(P["sharded_rank_with_two_clusters"]["plans"]) == 2
    fx = P["fx_bounds_kinds"]
    assert [p["pack24"] for p in fx["plans"]] == [1, 1, 0, 0, 0, 0] and fx["h_cshift"][0] == 6 and fx["h_cshift"][1] == 0
    assert not any(p["pack24"] for p in P["fx_bounds_none"]["plans"])
    assert all(p["prune"] for p in P["knob_seed_forced"]["plans"]) and P["knob_seed_forced"]["seed_chunks"] == 3
    assert P["knob_lanes_forced"]["NS"] == 3
    assert not any(p["psym"] for p in P["knob_panel_sym_0"]["plans"])
    assert not P["knob_panel_two_phase_0"]["two_phase"] and P["knob_panel_two_phase_0"]["NS"] == 2
    assert not any(p["psym"] for p in P["knob_panel_multi_launch_0"]["plans"]) and P["knob_panel_multi_launch_0"]["two_phase"]
    assert not any(p["flat"] for p in P["knob_flat_batch_0"]["plans"])
    assert not P["knob_prune_0"]["plans"][0]["prune"] and not P["knob_pack24_0"]["plans"][0]["pack24"] and not P["knob_cooc_pk_0"]["use_pk"]
    assert P["knob_coop_force"]["plans"][0]["coop"]
    assert P["no_lists_asked_for"]["plans"] == []
    assert P["forced_cooc_max_ch_64"]["error"] == 0 and P["forced_cooc_max_ch_64"]["plans"][0]["nch"] == 231      # widened to 256 columns
    e = P["error_forced_cooc_max_ch_64_panel_mode"]
    assert e["error"] == -10 and e["msg"] == "cluster 0: 30000 items need 469 column chunks (limit 255)"
    e = P["error_list_longer_than_topn_max"]
    assert e["error"] == -10 and e["msg"] == "min(numberOfRecommendations, items per cluster) = 3000 exceeds the top-N kernel limit 2048"
    e = P["error_count_balanced_without_pruned_cluster"]
    assert e["error"] == -9 and e["msg"] == "internal: count-balanced ownership without a cooperative cluster"


def test_invariants_the_scoring_flows_rely_on(planned):
    for name, j in planned.items():
        if j["error"]:
            continue
        in_group = {}
        for k, p in enumerate(j["plans"]):
            where = (name, k, p)
            assert p["nch"] < 256, where
            assert p["p_eff"] == p["Ic"] or (p["p_eff"] % 256 == 0 and p["tail_chunks"] < p["nch"]), where
            if p["psym"]:
                assert p["p_eff"] == p["panel_cols"], where
            if p["flat"]:
                assert not p["prune"] and not p["coop"] and not p["panel"], where
            if p["panel"]:
                need = p["Ic"] * p["panel_cols"] * 3 + p["Ic"] * p["ldb64"] * 7 + (p["b"] - p["a"]) * p["ldb64"] * 7 + p["Ic"] * p["nch"] * 12
                in_group.setdefault(j["group_of"][k], []).append(need)
            else:
                assert j["group_of"][k] == 0, where
        assert sorted(in_group) == list(range(len(in_group))) and (j["n_groups"] == max(1, len(in_group))), name
        if j["two_phase"]:      # no group is over its limit unless it holds a single cluster
            limit = 38500000000 if name == "c200_three_groups" else HBM // 3
            for g, needs in in_group.items():
                assert len(needs) == 1 or sum(needs) <= limit, (name, g, sum(needs), limit)
        assert len(j["group_of"]) == len(j["plans"]) and j["NS"] <= max(1, len(j["plans"])), name
        assert math.isfinite(sum(j["h_gscale"])), name
