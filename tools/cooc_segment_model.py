#!/usr/bin/env python3
"""Segment-fill model of the symmetric row walk, on the CPU.

The row kernel's cost is per SEGMENT (<= 64 entries of one rater's row slice in one column chunk), whatever the number of its lanes that
hold a pair.  This script counts, for a sample of synth.py's users, the segments and the pair visits of the two orientations of the walk:

  behind (CoocArgs::half == 1): a CSC entry (rater v, row i) walks v's slice of i's own chunk from the 64-aligned position in front of
      i, and v's whole slices of the chunks BEHIND i's chunk;
  front  (CoocArgs::half == 2): the own chunk likewise, and v's whole slices of the chunks IN FRONT of i's chunk.

Model: degrees and item weights of synth.py; the cells of a sampled user are drawn with numpy instead of the generator's hash (same
probabilities min(P_CAP, t_u w_r)); an item's column is its popularity RANK (the library orders columns by rater count); a user's CSR
row starts at a 64-aligned position.  Pair visits are the same for both orientations: an entry visits the entries behind it in its row.

    python tools/cooc_segment_model.py [--shape ml25m] [--sample 4000] [--max-ch 19968]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pick_chunks(n_items, max_ch):
    """fy_rm2_plan.hpp: pick_chunks."""
    if n_items <= max_ch:
        return -(-n_items // 64) * 64, 1
    cap = max_ch // 256 * 256
    nch = -(-n_items // cap)
    ch = min(cap, -(-(-(-n_items // nch)) // 256) * 256)
    return ch, -(-n_items // ch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--sample", type=int, default=4000)
    ap.add_argument("--max-ch", type=int, default=19968)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    synth = importlib.import_module("filmyou-core_amd.synth")
    n_users, n_items, nnz, _ = synth.SHAPES[args.shape]
    rng = np.random.Generator(np.random.PCG64(synth.SEED0))
    deg = synth._degrees(n_users, n_items, nnz, rng)
    w = 1.0 / np.arange(1, n_items + 1)          # by popularity rank = column
    w /= w.sum()
    t = synth._solve_t(deg, w)
    CH, nch = pick_chunks(n_items, args.max_ch)
    edges = np.arange(nch + 1) * CH
    pick = np.random.default_rng(args.seed)
    users = pick.choice(n_users, min(args.sample, n_users), replace=False)

    seg = {"own": 0, "behind": 0, "front": 0}
    lanes = {"own": 0, "behind": 0, "front": 0}      # useful lanes = pair visits
    hist_behind = np.zeros(65, dtype=np.int64)        # off-diagonal segments by active lanes
    hist_front = np.zeros(65, dtype=np.int64)
    share = np.zeros(nch)
    lengths = []
    for u in users:
        cols = np.flatnonzero(pick.random(n_items) < np.minimum(synth.P_CAP, t[u] * w))
        n = len(cols)
        lengths.append(n)
        if n == 0:
            continue
        co = np.searchsorted(cols, edges)             # chunk offsets of the row
        share += np.diff(co)
        pos = np.arange(n)
        own = cols // CH
        # own chunk: from the 64-aligned position in front of the entry (not in front of the slice) to the slice's end
        start = np.maximum(co[own], pos // 64 * 64)
        seg["own"] += int(((co[own + 1] - start + 63) // 64).sum())
        lanes["own"] += int((co[own + 1] - pos - 1).sum())
        per_chunk = np.diff(co)                       # slice lengths
        entries = per_chunk                           # entries of the row whose own chunk is c
        full, rest = per_chunk // 64, per_chunk % 64
        for a in range(nch):
            for b in range(a + 1, nch):
                # rectangle (rows of chunk a) x (columns of chunk b): walked by the entries of chunk a over the slice of b (behind),
                # or by the entries of chunk b over the slice of a (front)
                for key, hist, walkers, sl in (("behind", hist_behind, a, b), ("front", hist_front, b, a)):
                    k = int(entries[walkers])
                    seg[key] += k * int(full[sl] + (rest[sl] > 0))
                    lanes[key] += k * int(per_chunk[sl])
                    hist[64] += k * int(full[sl])
                    if rest[sl]:
                        hist[rest[sl]] += k
    scale = n_users / len(users)
    out = {"shape": args.shape, "sample": int(len(users)), "CH": int(CH), "nch": int(nch), "median_ratings": float(np.median(lengths)),
           "share_of_ratings_by_chunk": [round(float(x), 4) for x in share / share.sum()]}
    for key in ("own", "behind", "front"):
        out["segments_" + key] = float(seg[key] * scale)
        out["lanes_" + key] = round(lanes[key] / max(1, seg[key]), 2)
    for key, other in (("behind", hist_behind), ("front", hist_front)):
        total = seg["own"] + seg[key]
        out["segments_all_" + key] = float(total * scale)
        out["lanes_all_" + key] = round((lanes["own"] + lanes[key]) / max(1, total), 2)
        out["offdiag_share_le16_" + key] = round(float(other[:17].sum() / max(1, other.sum())), 4)
        out["offdiag_share_le32_" + key] = round(float(other[:33].sum() / max(1, other.sum())), 4)
    out["pair_visits"] = float((lanes["own"] + lanes["behind"]) * scale)
    out["segments_front_over_behind"] = round(out["segments_all_front"] / out["segments_all_behind"], 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
