"""Where a job's plan puts the row kernel's walk tables (csrc/fy_rm2_tables.hpp: layout_tables, host-only C++, built here with g++):
the chunk-offset range and the packed-CSR range of every planned cluster, its main segment-table descriptor, the tail descriptor of a
panel-mode cluster with tail rows, and every offset into the shared arrays.

Plans are fed to the function directly (one line per case, one `:`-separated record per plan), so that shapes plan_job gives only at
some size -- a cooperative plan between two local ones, a cluster without a CSC entry -- are one line each.  Everything asserted here is
a closed form of the INPUT; nothing is compared with another output of the function."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filmyou-core_amd", "csrc")

FIELDS = ["Uc", "sbase", "Ic", "CH", "nch", "q0", "nq", "coop", "half", "panel", "psym", "rect", "tail_chunks", "p_eff", "f0", "f1"]

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fy_rm2_tables.hpp"

static void print_csr(const fy::CsrDesc& d, bool first) {
    printf("%s{\"slot_base\": %d, \"n_slots\": %d, \"CH\": %d, \"nch\": %d, \"f0\": %d, \"f1\": %d, \"p_eff\": %d, \"has_tail\": %d, \"co_off\": %lld, \"co_tail_off\": %lld}",
           first ? "" : ", ", d.slot_base, d.n_slots, d.CH, d.nch, d.f0, d.f1, d.p_eff, d.has_tail, (long long)d.co_off, (long long)d.co_tail_off);
}
static void print_seg(const fy::SegDesc& d, bool first) {
    printf("%s{\"slot_base\": %d, \"q0\": %d, \"nq\": %d, \"nch\": %d, \"CH\": %d, \"half\": %d, \"rect\": %d, \"sym_rows\": %d, \"lim_from\": %d, \"lim_chunks\": %d, "
           "\"only_from\": %d, \"co_off\": %lld, \"cnt_off\": %lld}",
           first ? "" : ", ", d.slot_base, d.q0, d.nq, d.nch, d.CH, d.half, d.rect, d.sym_rows, d.lim_from, d.lim_chunks, d.only_from, (long long)d.co_off,
           (long long)d.cnt_off);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ls(line);
        std::string name, rec;
        if (!(ls >> name)) continue;
        std::vector<fy::Plan> plans;
        std::vector<int32_t> csr_range;
        while (ls >> rec) {
            std::vector<long long> v;
            std::stringstream rs(rec);
            std::string tok;
            while (std::getline(rs, tok, ':')) v.push_back(atoll(tok.c_str()));
            if (v.size() != 16) { fprintf(stderr, "%s: a plan has 16 fields\n", name.c_str()); return 2; }
            fy::Plan p{};
            p.c = (int)plans.size();
            p.Uc = (int32_t)v[0]; p.sbase = (int32_t)v[1]; p.Ic = (int32_t)v[2]; p.CH = (int32_t)v[3]; p.nch = (int32_t)v[4]; p.q0 = (int32_t)v[5]; p.nq = (int32_t)v[6];
            p.coop = v[7] != 0; p.half = v[8] != 0; p.panel = v[9] != 0; p.psym = v[10] != 0; p.rect = v[11] != 0;
            p.tail_chunks = (int32_t)v[12]; p.p_eff = (int32_t)v[13];
            plans.push_back(p);
            csr_range.push_back((int32_t)v[14]);
            csr_range.push_back((int32_t)v[15]);
        }
        csr_range.push_back(0);
        csr_range.push_back(0);
        try {
            const fy::TableLayout L = fy::layout_tables(plans, csr_range);
            printf("{\"name\": \"%s\", \"error\": 0, \"n_main\": %zu, \"co_total\": %lld, \"co_tail_total\": %lld, \"cnt_total\": %lld, \"main_of\": [", name.c_str(), L.n_main,
                   (long long)L.co_total, (long long)L.co_tail_total, (long long)L.cnt_total);
            for (size_t k = 0; k < L.main_of.size(); k++) printf(k ? ", %d" : "%d", L.main_of[k]);
            printf("], \"tail_of\": [");
            for (size_t k = 0; k < L.tail_of.size(); k++) printf(k ? ", %d" : "%d", L.tail_of[k]);
            printf("], \"csr\": [");
            for (size_t k = 0; k < L.csr.size(); k++) print_csr(L.csr[k], k == 0);
            printf("], \"seg\": [");
            for (size_t k = 0; k < L.seg.size(); k++) print_seg(L.seg[k], k == 0);
            printf("]}\n");
        } catch (const fy::PlanError& e) {
            printf("{\"name\": \"%s\", \"error\": %d, \"msg\": \"%s\"}\n", name.c_str(), e.code, e.msg.c_str());
        }
    }
    return 0;
}
'''


def plan(Uc, Ic, CH, nch, nq, coop=0, half=0, panel=0, psym=0, rect=0, tail_chunks=0, p_eff=None):
    return dict(Uc=Uc, Ic=Ic, CH=CH, nch=nch, nq=nq, coop=coop, half=half, panel=panel, psym=psym, rect=rect, tail_chunks=tail_chunks,
                p_eff=Ic if p_eff is None else p_eff)


def place(plans):
    """slots, CSC entries and CSR entries of the clusters one behind the other (the CSR of a cluster is as long as its CSC)"""
    s = q = 0
    for p in plans:
        p.update(sbase=s, q0=q, f0=q, f1=q + p["nq"])
        s += p["Uc"]
        q += p["nq"]
    return plans


PANEL = dict(Ic=30000, CH=4096, nch=8, panel=1)
CASES = {
    "one_cluster_half_rect": [plan(162541, 59047, 19712, 3, 25000095, half=1, rect=1)],
    "one_cluster_one_chunk": [plan(9000, 8000, 8000, 1, 700000, half=1)],
    # panel mode without the symmetric panel; the second and the fourth cluster fit one chunk: no tail rows
    "five_panels_two_without_tail": [plan(3250, nq=500000 + k, tail_chunks=1, p_eff=4096, **PANEL) if k % 2 == 0 else plan(3000, 4000, 4096, 1, 90000 + k, panel=1)
                                     for k in range(5)],
    "symmetric_panels": [plan(3250 + k, nq=480000 + 7 * k, psym=1, tail_chunks=2, p_eff=8192, **PANEL) for k in range(4)],
    "cooperative_plan_in_the_middle": [plan(700, 9000, 9216, 1, 60000, half=1), plan(20000, 20000, 19968, 2, 2000000, coop=1),
                                       plan(3250, nq=500000, psym=1, tail_chunks=1, p_eff=4096, **PANEL), plan(900, 5000, 5056, 1, 80000)],
    "a_cluster_without_entries": [plan(800, 9000, 9216, 1, 70000, half=1), plan(5, 3, 64, 1, 0), plan(3250, nq=500000, tail_chunks=1, p_eff=4096, **PANEL)],
    "a_half_walk_that_must_not_be_rect": [plan(3250, 30000, 4096, 8, 500000, half=0, rect=1)],
    # three tables of three chunks: 9 x 238 609 292 = 2 147 483 628 prefix entries is the largest total the limit lets through; one more
    # CSC entry in one of them is three entries too many
    "just_below_the_prefix_limit": [plan(1000, 59047, 19712, 3, 238609291) for _ in range(3)],
    "error_prefix_entries": [plan(1000, 59047, 19712, 3, 238609291) for _ in range(2)] + [plan(1000, 59047, 19712, 3, 238609292)],
}


@pytest.fixture(scope="module")
def laid_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("rm2_tables")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = str(d / "drv")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(src)], check=True)
    lines = [name + " " + " ".join(":".join(str(p[f]) for f in FIELDS) for p in place(plans)) for name, plans in CASES.items()]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [json.loads(line) for line in r.stdout.splitlines()]
    assert [g["name"] for g in got] == list(CASES)
    return {g["name"]: g for g in got}


def good(laid_out):
    return [(name, CASES[name], laid_out[name]) for name in CASES if not name.startswith("error_")]


def has_tail(p):
    return not p["coop"] and p["p_eff"] < p["Ic"]


def test_chunk_offset_ranges_are_contiguous_in_plan_order(laid_out):
    for name, plans, L in good(laid_out):
        at = at_tail = 0
        for p, d in zip(plans, L["csr"]):
            assert (d["co_off"], d["co_tail_off"]) == (at, at_tail), name
            assert (d["slot_base"], d["CH"], d["nch"], d["f0"], d["f1"], d["p_eff"]) == (p["sbase"], p["CH"], p["nch"], p["f0"], p["f1"], p["p_eff"]), name
            # a cooperative plan keeps its packed-CSR range and has no chunk offsets here: its ranks build their own
            assert d["n_slots"] == (0 if p["coop"] else p["Uc"]) and d["has_tail"] == int(has_tail(p)), name
            at += d["n_slots"] * (p["nch"] + 1)
            at_tail += 2 * p["Uc"] if has_tail(p) else 0
        assert (L["co_total"], L["co_tail_total"]) == (at, at_tail), name
        assert len(L["csr"]) == len(plans), name


def test_count_ranges_main_tables_then_tail_tables(laid_out):
    for name, plans, L in good(laid_out):
        local = [k for k, p in enumerate(plans) if not p["coop"]]
        tails = [k for k in local if has_tail(plans[k])]
        assert L["n_main"] == len(local) and len(L["seg"]) == len(local) + len(tails), name
        assert L["main_of"] == [local.index(k) if k in local else -1 for k in range(len(plans))], name      # cooperative plans have no table
        assert L["tail_of"] == [len(local) + tails.index(k) if k in tails else -1 for k in range(len(plans))], name      # a tail table exactly where p_eff < Ic
        at = 0
        for k in local:
            d = L["seg"][L["main_of"][k]]
            assert d["cnt_off"] == at and d["nch"] == plans[k]["nch"], (name, k)
            at += plans[k]["nch"] * (plans[k]["nq"] + 1)
        for k in tails:
            d = L["seg"][L["tail_of"][k]]
            assert d["cnt_off"] == at and d["nch"] == 1, (name, k)
            at += plans[k]["nq"] + 1
        assert L["cnt_total"] == at and at + 1 < 0x7FFFFFF0, name


def test_descriptors_say_what_the_plan_says(laid_out):
    """The rules of the all-clusters build this function was split from: a table is cut (half) for the symmetric walk and for the
    symmetric panel; the symmetric panel cuts only the head rows (sym_rows = p_eff) and limits every row (lim_from = 0) to the panel's
    chunks, the plain panel limits the tail rows (lim_from = p_eff); the limit is tail_chunks where the cluster has tail rows, else off;
    rect only with a cut; a tail table is one uncut chunk over the tail rows' entries (only_from = p_eff) of the block-compressed CSR."""
    for name, plans, L in good(laid_out):
        for k, p in enumerate(plans):
            if p["coop"]:
                continue
            d = L["seg"][L["main_of"][k]]
            assert (d["slot_base"], d["q0"], d["nq"], d["CH"], d["only_from"]) == (p["sbase"], p["q0"], p["nq"], p["CH"], 0), (name, k)
            assert d["co_off"] == L["csr"][k]["co_off"], (name, k)
            half = int(bool(p["half"] or p["psym"]))
            assert d["half"] == half and d["rect"] == int(bool(half and p["rect"])), (name, k)
            assert d["sym_rows"] == (p["p_eff"] if p["psym"] else 0), (name, k)
            assert d["lim_from"] == (0 if p["psym"] else p["p_eff"]), (name, k)
            assert d["lim_chunks"] == (p["tail_chunks"] if p["panel"] and p["tail_chunks"] > 0 and p["p_eff"] < p["Ic"] else 0), (name, k)
            if has_tail(p):
                t = L["seg"][L["tail_of"][k]]
                assert (t["slot_base"], t["q0"], t["nq"], t["only_from"], t["co_off"]) == (p["sbase"], p["q0"], p["nq"], p["p_eff"], L["csr"][k]["co_tail_off"]), (name, k)
                assert (t["half"], t["rect"], t["sym_rows"], t["lim_from"], t["lim_chunks"]) == (0, 0, 0, 0, 0), (name, k)


def test_the_cases_are_what_they_are_named_for(laid_out):
    one = laid_out["one_cluster_half_rect"]
    assert one["n_main"] == 1 and one["seg"][0]["half"] == 1 and one["seg"][0]["rect"] == 1 and one["co_total"] == 162541 * 4
    assert laid_out["one_cluster_one_chunk"]["cnt_total"] == 700001
    assert laid_out["five_panels_two_without_tail"]["tail_of"] == [5, -1, 6, -1, 7]
    assert all(d["sym_rows"] == 8192 and d["lim_chunks"] == 2 for d in laid_out["symmetric_panels"]["seg"][:4])
    assert laid_out["cooperative_plan_in_the_middle"]["main_of"] == [0, -1, 1, 2]
    assert laid_out["a_cluster_without_entries"]["seg"][1]["nq"] == 0 and laid_out["a_cluster_without_entries"]["seg"][2]["cnt_off"] == 70001 + 1
    assert laid_out["a_half_walk_that_must_not_be_rect"]["seg"][0]["rect"] == 0


def test_more_prefix_entries_than_the_scan_holds_are_refused(laid_out):
    total = 3 * 3 * 238609292
    assert laid_out["just_below_the_prefix_limit"]["cnt_total"] == total and total + 1 < 0x7FFFFFF0 <= total + 3 + 1
    e = laid_out["error_prefix_entries"]
    assert e["error"] == -10 and e["msg"] == "segment tables of 3 clusters need %d prefix entries (limit 2^31)" % (total + 3)
