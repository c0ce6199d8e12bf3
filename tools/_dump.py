"""`--dump DIR` of the item-CF request tools: every array of a result as DIR/<name>.<column>.npy, in the order the call returned it,
and DIR/stats.json with the integer fields of its statistics (the timings, the only floats, are left out).  Two builds of the library
are compared byte for byte that way, as with tools/itemsim_request_bench.py --dump.  A name is written once: its first result."""
import json
import os

import numpy as np


class Dump:
    def __init__(self, directory):
        self.dir, self.stats = directory, {}

    def __call__(self, name, res, *stats):
        """res: a result with rows() (and pairs() where it has the per-pair view); stats: its dicts of statistics"""
        if not self.dir or name in self.stats:
            return
        os.makedirs(self.dir, exist_ok=True)
        views = [("", res.rows())] + ([("pairs.", res.pairs())] if hasattr(res, "pairs") else [])
        for prefix, cols in views:
            for col, arr in cols.items():
                np.save(os.path.join(self.dir, "%s.%s%s.npy" % (name, prefix, col)), arr)
        whole = lambda v: isinstance(v, int) or (isinstance(v, list) and all(isinstance(x, int) for x in v))
        self.stats[name] = {k: v for d in stats + (res.stats,) for k, v in d.items() if whole(v)}
        with open(os.path.join(self.dir, "stats.json"), "w") as f:
            json.dump(self.stats, f, indent=1, sort_keys=True)
