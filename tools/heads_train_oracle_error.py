"""The fp32 CPU oracle's own error, which fixes the gates of tests/test_gpu_heads_train.py: the reference-structured head as a
torch nn.Sequential in fp32 on the CPU against the same in float64, per case and quantity (the raw map, the activated map, every
layer's weight and bias gradient), as max|v32 - v64| / max|v64|, and the gate tests/heads_train_ref.case_gate derives from it.
The cases are those of tests/heads_train_ref.py: CASES, then REPLICATED (the map on the base case, the gradients on the batch of just
the images that carry a dY).  Ends with the worst quantity of each case, the table of the GPU test's docstring.  No GPU, no library.    python tools/heads_train_oracle_error.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import heads_train_ref as T


def main():
    import math
    worst = {}
    labels = ["y", "out"] + [f"g{k}{l}" for l in range(4) for k in "wb"]
    print(f"{'case':22s}" + "".join(f"{n:>10s}" for n in labels))
    for name in T.CASES:
        e = T.oracle_errors(name)
        print(f"{name:22s}" + "".join(f"{e[n]:10.1e}" if n in e else f"{'-':>10s}" for n in labels))
        print(f"{'    its gates':22s}" + "".join(f"{T.case_gate(e[n]):10.1e}" if n in e else f"{'-':>10s}" for n in labels))
        c = T.build(name)
        what = "max sum|terms|/resolution (log2)" if c["family"] == "dyadic" else "min hidden pre-activation"
        vals = [f"{math.log2(v):.1f}" if c["family"] == "dyadic" else f"{v:.2f}" for v in c["checks"]]
        print(f"{'    ' + what:22s}  " + " ".join(vals))
        worst[name] = max(e.items(), key=lambda kv: kv[1])
    for name in T.REPLICATED:
        e = T.rep_oracle_errors(name)
        g = T.rep_geometry(name)
        print(f"{name:22s}" + "".join(f"{e[n]:10.1e}" if n in e else f"{'-':>10s}" for n in labels))
        print(f"{'    its gates':22s}" + "".join(f"{T.case_gate(e[n]):10.1e}" if n in e else f"{'-':>10s}" for n in labels))
        print(f"    M {g['M']}, chunks {g['chunks']} of {g['chunk']}, {g['tiles']} tiles, {g['out_elems']} output elements, "
              f"{g['active']} list positions")
        worst[name] = max(e.items(), key=lambda kv: kv[1])
    print()
    cells = [f"{n:21s} {v:.1e} ({k})" for n, (k, v) in worst.items()]
    for i in range(0, len(cells), 3):
        print("    " + "   ".join(f"{c:36s}" for c in cells[i:i + 3]).rstrip())


if __name__ == "__main__":
    main()
