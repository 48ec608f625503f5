"""Records what the pose engine plans and launches, through the C-ABI, as tests/golden/plan_matrix.json:

    python tools/dump_plan.py OUT.json [--parent HASH]        (library: the in-tree one, or FLOPE_AMD_LIB)

Per case (crop size, max_batch = batch, dtype, option list): describe_plan() and launches(); for "forward" cases one forward on
a torch.rand input followed by launch_info(batch) -- layer (with the launch's detail) and kernel label per launch.  "plan" cases
record the plan text and the launch count only.  The option probe sets every option to each of PROBE_VALUES and reads the stored
value back (set_option returns the previous value).  tests/test_host.py holds the CPU planner (csrc/plan.h) to this file and
tests/test_gpu_parity.py a live engine; the file is recorded from the commit BEFORE a change of the planner, never from the code
under test.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

OPTIONS = ["patch", "bm256", "persist", "rows_grid", "split", "fc1_packed", "w4mtlo", "lag", "w4mt", "fc2_k4", "ksplit", "stem_r",
           "stem_persist", "rowseg", "skew", "r4", "s1r", "s2r_grid", "s2r", "w4", "w4cw", "w4cwf", "prio", "reslds", "gstag", "dsfuse",
           "stag", "streams", "fuse_stem", "ldspad", "dbg", "nbuf", "profile"]
PROBE_VALUES = [-5, -1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 64, 100, 196, 600]
MFMA_SETS = [dict(patch=1, bm256=1, nbuf=3, fuse_stem=1, stag=2, stem_persist=2, reslds=0, prio=2), dict(patch=0, bm256=0, nbuf=3, fuse_stem=0, stag=0),
             dict(patch=1, bm256=0, nbuf=2, fuse_stem=0, stag=0), dict(patch=0, bm256=1, nbuf=2, fuse_stem=1, stag=1, dsfuse=0, gstag=0, stem_persist=0, skew=0, prio=1)]


def matrix():
    """[(kind, H, W, B, dtype, [(option, value)])]: forwards only where the GPU suite already runs that combination."""
    from test_gpu_conv_elementwise import CASES
    out = []

    def add(kind, H, W, B, dtype, opts):
        c = (kind, H, W, B, dtype, sorted(opts.items()))
        if c not in out:
            out.append(c)

    for H, W, B, dtype, _fmt, _nb, opts in CASES:
        add("forward", H, W, B, dtype, dict(opts))
    # test_conflict_free_patch_image_and_4_wave_kernel_do_not_change_a_bit
    for H, W, B, dtype in [(224, 224, 64, "f16"), (224, 224, 19, "f16"), (224, 224, 32, "bf16"), (200, 136, 7, "f16"), (512, 512, 2, "f16")]:
        cfgs = [dict(w4mt=7, w4cw=0), dict(w4mt=8), dict(w4mt=0, w4cw=0), dict(w4mt=6), dict(w4mt=5), dict(w4cw=4, w4cwf=2), dict(w4cw=4, w4cwf=3, streams=2), dict(w4=0)]
        if (H, W) != (224, 224):
            cfgs = [dict(w4mt=7, w4cw=0), dict(w4mt=8), dict(w4mt=0, w4cw=0), dict(), dict(w4=0)]
        for cfg in cfgs:
            add("forward", H, W, B, dtype, {**dict(streams=1, ksplit=0, s1r=0), **cfg})
    # test_mfma_path_every_stage_vs_emulating_oracle
    for dtype in ("f16", "bf16"):
        for o in MFMA_SETS:
            for H, W, B in [(224, 224, 5), (96, 80, 3), (65, 71, 2)]:
                add("forward", H, W, B, dtype, o)
    # the two layer-2 tests (conv_s2r / conv_s1r against the kernels they replace)
    for B, dtype, streams in [(3, "f16", 1), (40, "bf16", 1), (150, "f16", 2)]:
        for name in ("s2r", "s1r"):
            for v in (1, 0):
                add("forward", 224, 224, B, dtype, {name: v, "streams": streams})
    add("forward", 224, 224, 3, "f16", dict(dsfuse=0, streams=1))
    add("forward", 96, 80, 2, "f16", {})
    # options no GPU test sets: the plan, not a forward
    for B in (256, 40):
        for o in (dict(persist=1), dict(rows_grid=-1), dict(rows_grid=64), dict(gstag=2), dict(s2r_grid=128), dict(streams=3), dict(streams=4)):
            add("plan", 224, 224, B, "f16", o)
    add("plan", 512, 512, 16, "f16", dict(persist=1))
    add("plan", 512, 512, 16, "f16", dict(gstag=2))
    return out


def record(case, sd):
    from flope_amd.engine import PoseEngine
    kind, H, W, B, dtype, opts = case
    e = PoseEngine(H, W, B, dtype)
    for k, v in opts:
        e.set_option(k, v)
    e.load_state_dict(sd)
    rec = dict(kind=kind, H=H, W=W, batch=B, dtype=dtype, opts=[[k, v] for k, v in opts], plan=e.describe_plan(), launches=e.launches())
    if kind == "forward":
        torch.manual_seed(3)
        e.forward(torch.rand(B, 3, H, W).cuda())
        torch.cuda.synchronize()
        rec["info"] = [[layer, k] for layer, k, _ in e.launch_info(B)]
    e.close()
    return rec


def probe():
    from flope_amd.engine import PoseEngine
    e = PoseEngine(224, 224, 1, "f16")
    out = {}
    raw = lambda name, v: e.lib.flope_set_option(e.handle, name.encode(), v)   # (a stored negative value is no error: not PoseEngine.set_option)
    for name in OPTIONS:
        default = raw(name, 0)
        raw(name, default)
        stored = []
        for v in PROBE_VALUES:
            raw(name, v)
            stored.append(raw(name, default))
        out[name] = dict(default=default, stored=stored)
    unknown = raw("no_such_option", 1)
    e.close()
    return out, unknown


def main():
    from flope_amd.weights import synthetic_state_dict
    out_path = sys.argv[1]
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else ""
    sd = synthetic_state_dict(0)
    doc = dict(parent=parent, num_cus=torch.cuda.get_device_properties(0).multi_processor_count, probe_values=PROBE_VALUES,
               cases=[])
    doc["probe"], doc["unknown_option"] = probe()
    for case in matrix():
        doc["cases"].append(record(case, sd))
        print(len(doc["cases"]), case, flush=True)
    save(doc, out_path)


def save(doc, path):
    """Writes the record with every distinct plan line and (layer, kernel) pair stored once (`plan_lines`, `launch_rows`); a case
    refers to them by index.  One line per table entry, probe and case."""
    doc = dict(doc)
    plan_lines, rows, cases = [], [], []

    def index(table, item):
        if item not in table:
            table.append(item)
        return table.index(item)

    for c in doc["cases"]:
        c = dict(c, plan=[index(plan_lines, ln) for ln in c["plan"].split("\n")])
        if "info" in c:
            c["info"] = [index(rows, r) for r in c["info"]]
        cases.append(c)
    one = lambda v: json.dumps(v, separators=(",", ":"))
    block = lambda items: "[\n" + ",\n".join(one(v) for v in items) + "\n]"
    head = {k: doc[k] for k in ("parent", "num_cus", "probe_values", "unknown_option")}
    with open(path, "w") as f:
        f.write("{" + one(head)[1:-1] + ',\n"probe":{\n' + ",\n".join(f"{one(k)}:{one(v)}" for k, v in doc["probe"].items()) + "\n},\n"
                + f'"plan_lines":{block(plan_lines)},\n"launch_rows":{block(rows)},\n"cases":{block(cases)}}}\n')


def load(path):
    """The record as main() built it: every case with its plan text and, for "forward" cases, info = [[layer, kernel]]."""
    with open(path) as f:
        doc = json.load(f)
    for c in doc["cases"]:
        c["plan"] = "\n".join(doc["plan_lines"][i] for i in c["plan"])
        if "info" in c:
            c["info"] = [doc["launch_rows"][i] for i in c["info"]]
    return doc


if __name__ == "__main__":
    main()
