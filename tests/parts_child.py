"""One part of a merge over partitioned records in a process of its own: the child that tests/test_gpu_parts_processes.py starts (not a test
module).  Usage: python parts_child.py SPEC.json

SPEC = {"part": g, "parts": n, "out": directory, "merges": [{"group": name, "a": prefix, "b": prefix, "kmer": k, "knobs": {name: value}}, ...]}.
An input prefix names <prefix>_data.npy (native bytes), <prefix>_cum.npy (cumulative samples) and <prefix>.json (sequences, bases).  The child
binds GPU 0 and runs the merges in order; merges that name the same group run on one bwtm_group.  It writes <out>/part<g>_<k>_{data,be,cum}.npy
of every merge that succeeded and <out>/part<g>.json: per merge byte_offset, total_nbytes, next_block_start, stats and seconds, or the
bwtm error code and message.  A merge that fails frees its group; later merges that name it are not run.  Exit status 0 means every record was
written."""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# what every merge of a child starts from (the knobs' defaults)
KNOB_DEFAULTS = {"range_ratio": 8, "frontier_epoch": 0, "part_capacity": 0}


def main(spec_path):
    import numpy as np
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import capi, partitioned
    with open(spec_path) as f:
        spec = json.load(f)
    g, parts, out = int(spec["part"]), int(spec["parts"]), spec["out"]
    pkg.init(0)

    def load(prefix):
        with open(prefix + ".json") as f:
            meta = json.load(f)
        return capi.host_index(np.load(prefix + "_data.npy"), np.load(prefix + "_cum.npy"), meta["sequences"], meta["bases"])

    groups, records = {}, []
    for k, m in enumerate(spec["merges"]):
        rec = {"merge": k}
        t0 = time.monotonic()
        name = m["group"]
        if name in groups and groups[name] is None:
            rec.update(code=None, error="not run: its group failed in an earlier merge")
            records.append(rec)
            continue
        try:
            a, b = load(m["a"]), load(m["b"])
            if name not in groups:
                groups[name] = capi.Group(name, g, parts)
            for key, v in m.get("knobs", {}).items():
                pkg.tune(key, v)
            try:
                S, stats = partitioned.merge_part(groups[name], a, b, kmer=int(m["kmer"]))
            finally:
                for key in m.get("knobs", {}):
                    pkg.tune(key, KNOB_DEFAULTS[key])
            try:
                data, be, cum = partitioned.slice_arrays(S)
                rec.update(byte_offset=S.byte_offset, total_nbytes=S.total_nbytes, next_block_start=S.next_block_start, stats=stats)
            finally:
                S.free()
            for tag, arr in (("data", data), ("be", be), ("cum", cum)):
                np.save(os.path.join(out, "part%d_%d_%s.npy" % (g, k, tag)), arr)
        except pkg.BwtmError as e:
            got = re.match(r"bwtm error (\d+): (.*)", str(e), re.S)
            rec.update(code=int(got.group(1)) if got else None, error=got.group(2) if got else str(e))
            if groups.get(name) is not None:
                groups[name].abort(); groups[name].free()
            groups[name] = None
        rec["seconds"] = time.monotonic() - t0
        records.append(rec)
    for grp in groups.values():
        if grp is not None:
            grp.free()
    with open(os.path.join(out, "part%d.json" % g), "w") as f:
        json.dump(records, f)


if __name__ == "__main__":
    main(sys.argv[1])
