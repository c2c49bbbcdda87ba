"""GPU probe behind two figures of DESIGN.md §4.5: values that tests/test_gpu_hot_values.py cannot tell apart.

    python tools/fastpath_probe.py OUT.npz                 (SR_AMD_LIB picks the library build)
    python tools/fastpath_probe.py OUT.npz --compare OTHER.npz

Float32, through PRED (whose 4 rows per lane take the same row bodies as the loss builds):
  div  x1 / x2 on 2^20 drawn pairs (those representable: about 725,000) whose exact quotient lies 2^-24 .. 2^-25 ulp
       from a rounding midpoint, divisors over the whole binade [1, 2) (the construction of the test's
       _hard_quotients with a random odd B): printed, the number that differ from IEEE division (numpy);
  exp  2,048 arguments of [-89, -88) in one call and 96 of (88, 89] one row per call (results near floatmax; the
       neighbours of the overflow threshold among them), as exp(x1) and exp(x1 * x2): their bits are saved.
With --compare, the number of saved values (quotients and exponentials) that differ from another build's.  A build
without sr_div_rows_f32's second correction step, and one whose sr_exp_rows_f32 tests |x| <= 89, differ from this
one in none (MI355X, ROCm 7.2.0).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "symbolicregression.jl_amd")]

from sr_amd import Dataset, Options, batch, eval_tree_array_batch, flatten_trees, parse_expression  # noqa: E402

OPTS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])


def near_midpoint_pairs(n, seed=5):
    rng = np.random.default_rng(seed)
    M = 1 << 24
    a, b = [], []
    for B, r in zip((rng.integers(1 << 22, 1 << 23, n) * 2 + 1).tolist(), rng.choice([1, -1], n).tolist()):
        Q = (r * pow(B, -1, M)) % M + M
        A = (B * Q - r) >> 24
        if A < M or A % 2 == 0:  # the dividend is a Float32
            a.append(A * 2.0 ** -23)
            b.append(B * 2.0 ** -23)
    m = len(a) // 4096 * 4096
    return np.array(a[:m], dtype=np.float32), np.array(b[:m], dtype=np.float32)


def main():
    out_path = sys.argv[1]
    opts = Options(**OPTS)
    a, b = near_midpoint_pairs(1 << 20)
    ds = Dataset(np.stack([a, b]))
    q, comp = eval_tree_array_batch(flatten_trees([parse_expression("x1 / x2", opts)], np.float32), ds, opts)
    ds.free_device()
    assert comp[0]
    print("div:", len(a), "pairs,", int((q[0].view(np.uint32) != (a / b).view(np.uint32)).sum()), "differ from IEEE division")
    rng = np.random.default_rng(89)
    x = np.nextafter(rng.uniform(88, 89, 4096).astype(np.float32), np.float32(90))
    x[:2048] *= -1
    x[2048:2052] = [88.72283, 88.72284, 88.72285, 89.0]
    ds = Dataset(np.stack([x, np.ones_like(x)]))
    tb = flatten_trees([parse_expression("exp(x1)", opts), parse_expression("exp(x1 * x2)", opts)], np.float32)
    e, comp = eval_tree_array_batch(tb, batch(ds, np.arange(2048)), opts)
    assert comp.all()
    pos = []
    for k in range(2048, 2048 + 96):
        o, c = eval_tree_array_batch(tb, batch(ds, np.array([k])), opts)
        pos.append(np.where(c, o[:, 0], np.float32(np.inf)))  # incomplete: the value overflowed
    ds.free_device()
    e = np.concatenate([e, np.array(pos, dtype=np.float32).T], axis=1)
    print("exp:", e.size, "values saved")
    np.savez(out_path, div=q[0], exp=e)
    if "--compare" in sys.argv:
        other = np.load(sys.argv[sys.argv.index("--compare") + 1])
        for key, v in (("div", q[0]), ("exp", e)):
            print(key, "differing from the other build:", int((v.view(np.uint32) != other[key].view(np.uint32)).sum()), "of", v.size)


if __name__ == "__main__":
    main()
