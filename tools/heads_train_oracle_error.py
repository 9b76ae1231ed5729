"""The fp32 CPU oracle's own error, which fixes the gates of tests/test_gpu_heads_train.py: the reference-structured head as a
torch nn.Sequential in fp32 on the CPU against the same in float64, per case and quantity (the raw map, the activated map, every
layer's weight and bias gradient), as max|v32 - v64| / max|v64|, and the gate tests/heads_train_ref.case_gate derives from it.
The cases are those of tests/heads_train_ref.py.  No GPU, no library.    python tools/heads_train_oracle_error.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import heads_train_ref as T


def main():
    labels = ["y", "out"] + [f"g{k}{l}" for l in range(4) for k in "wb"]
    print(f"{'case':22s}" + "".join(f"{n:>10s}" for n in labels))
    for name in T.CASES:
        e = T.oracle_errors(name)
        print(f"{name:22s}" + "".join(f"{e[n]:10.1e}" if n in e else f"{'-':>10s}" for n in labels))
        print(f"{'    its gates':22s}" + "".join(f"{T.case_gate(e[n]):10.1e}" if n in e else f"{'-':>10s}" for n in labels))
        c = T.build(name)
        what = "max sum|terms|/resolution (log2)" if c["family"] == "dyadic" else "min hidden pre-activation"
        import math
        vals = [f"{math.log2(v):.1f}" if c["family"] == "dyadic" else f"{v:.2f}" for v in c["checks"]]
        print(f"{'    ' + what:22s}  " + " ".join(vals))


if __name__ == "__main__":
    main()
