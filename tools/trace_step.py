"""One bench step out of a rocprofv3 kernel trace: launches and time per
kernel family, and how long the step's first factor and first solve wait
for what runs in front of them.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME \
        -- python bench.py --steps 3 --warmup 1
    python tools/trace_step.py DIR/NAME_kernel_trace.csv [chunks per step]

A step is taken as one period of the launch sequence: from behind the
last solve launch of one step to the last solve launch of the next (the
pulsar sum of a step's last chunk is counted with the following step).
The period reported is the last whole one, a graph replay of the timed
region.  Chunks per step: ceil(draws / draw chunk), 10 for the defaults.
"""

import collections
import csv
import re
import sys

FAMILIES = [
    ("solve (trsm_fp_draws)", r"trsm_fp_draws_kernel"),
    ("factor (chol_batch)", r"chol_batch_kernel"),
    ("phi_inv_batch", r"phi_inv_batch_kernel"),
    ("torch pow", r"pow_tensor"),
    ("torch reciprocal", r"reciprocal_kernel"),
    ("torch cat/stack", r"CatArrayBatchedCopy"),
    ("torch reduce (pulsar sum)", r"reduce_kernel"),
    ("torch copy", r"direct_copy_kernel"),
    ("torch fill", r"FillFunctor"),
    ("torch mul/div by scalar", r"[AB]UnaryFunctor"),
    ("torch mul", r"MulFunctor"),
    ("torch div", r"DivFunctor"),
    ("torch add/sub", r"CUDAFunctor(OnSelf)?_add"),
    ("runtime buffer copy (input rotation)", r"__amd_rocclr_copyBuffer"),
]


def family(name):
    for label, pat in FAMILIES:
        if re.search(pat, name):
            return label
    return "other: " + name[:50]


def main():
    path = sys.argv[1]
    chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        r["t0"], r["t1"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    rows.sort(key=lambda r: r["t0"])
    solves = [i for i, r in enumerate(rows)
              if "trsm_fp_draws_kernel" in r["Kernel_Name"]]
    nstep = len(solves) // chunks
    assert nstep >= 2, "need two steps' solve launches in the trace"
    seg = rows[solves[(nstep - 1) * chunks - 1] + 1:solves[nstep * chunks - 1] + 1]
    start = seg[0]["t0"]
    print(f"{len(seg)} launches in the step, "
          f"{(seg[-1]['t1'] - start) / 1e6:.2f} ms from its first launch to "
          "the end of its last solve")
    agg = collections.OrderedDict()
    for r in seg:
        a = agg.setdefault(family(r["Kernel_Name"]), [0, 0])
        a[0] += 1
        a[1] += r["t1"] - r["t0"]
    for k, (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"  {k:40s} {n:4d} launches {t / 1e6:9.3f} ms")
    other = sum(t for k, (n, t) in agg.items()
                if not k.startswith(("solve", "factor")))
    print(f"  everything but solve and factor: {other / 1e6:.3f} ms")
    # the previous step's last pulsar sum and the input rotation's copies
    # lead the period; the step proper starts behind the last such copy
    iscopy = ["copyBuffer" in r["Kernel_Name"] for r in seg]
    i = iscopy.index(True) if True in iscopy else 0
    while i < len(seg) - 1 and iscopy[i]:
        i += 1
    first = seg[i]
    for label, pat in (("factor", "chol_batch_kernel"),
                       ("solve", "trsm_fp_draws_kernel")):
        k = next(r for r in seg if pat in r["Kernel_Name"])
        print(f"first {label} starts {(k['t0'] - first['t0']) / 1e6:.3f} ms "
              f"after the step's first kernel ({family(first['Kernel_Name'])})")


if __name__ == "__main__":
    main()
