"""The fp32 oracle's own backward error, which fixes the gates of tests/test_gpu_deform_conv2d_backward.py: autograd through
oracle/dcn_ref.deform_conv2d in fp32 on the CPU against the same in float64, per case and gradient, as
max|g32 - g64| / max|g64|; then the same for the DeformConv call sequence.  The cases are those of tests/dcn_backward_ref.py.
No GPU, no library.    python tools/dcn_backward_oracle_error.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from oracle import dcn_ref
from tests import dcn_backward_ref as T


def gate(worst):
    return 5e-6 if worst <= 2.5e-6 else 2 * worst


def main():
    """the first six cases share one gate per gradient (from their worst error); each later case has its own (T.case_gate)"""
    worst = {n: 0.0 for n in T.NAMES}
    print(f"{'case (B,Cin,Cout,H,W,scale,mask)':40s}" + "".join(f"{n:>10s}" for n in T.NAMES))
    for i, case in enumerate(T.CASES):
        if i == T.NEW_CASES[0]:
            print(f"{'worst':40s}" + "".join(f"{worst[n]:10.1e}" for n in T.NAMES))
            print(f"{'gate':40s}" + "".join(f"{gate(worst[n]):10.1e}" for n in T.NAMES))
        args = T.make_case(i)
        g64, g32 = T.oracle_grads(*args), T.oracle_grads(*args, dtype=torch.float32)
        row, gates = [], []
        for n in T.NAMES:
            if g64[n] is None:
                row.append(f"{'-':>10s}")
                gates.append(f"{'-':>10s}")
                continue
            e = T.relerr(g32[n], g64[n])
            if i not in T.NEW_CASES:
                worst[n] = max(worst[n], e)
            else:
                gates.append(f"{T.case_gate(e):10.1e}")
            row.append(f"{e:10.1e}")
        print(f"{str(case):40s}" + "".join(row))
        if i in T.NEW_CASES:
            print(f"{'    its gate':40s}" + "".join(gates))

    g64 = T.sequence_grads(dcn_ref.deform_conv2d, "cpu", torch.float64)[0]
    g32 = T.sequence_grads(dcn_ref.deform_conv2d, "cpu", torch.float32)[0]
    errs = [T.relerr(a, b) for a, b in zip(g32, g64)]
    print(f"\n{'DeformConv sequence ' + str(T.SEQ_SHAPE):40s}" + "".join(f"{n:>10s}" for n in T.SEQ_NAMES))
    print(f"{'fp32 graph against float64':40s}" + "".join(f"{e:10.1e}" for e in errs))
    print(f"{'gate':40s}" + "".join(f"{gate(e):10.1e}" for e in errs))


if __name__ == "__main__":
    main()
