"""CPU simulation of the loss launch's candidate binades: which (tree, row block) pairs
the plan could NOT take from the candidates, i.e. what is left to the FOLD pass, under different guesses
of the running sum at a row block.  tools/r06_fold_cand.py's method (the oracle's predictions, f64 block
sums, the plan's window delta) at the device's real block size:

* "none possible": the blocks the plan itself calls slow (the first block, and every block whose window
  [prefix before (1 - delta), prefix after (1 + delta)] meets a binade edge) — no guess can take those;
* "first tile": the block's first tile's sum x tiles per block x rb (fold_cand_est 0);
* "prefix, lag L": the sum of the blocks finished L blocks ago, scaled by rb / (rb - L) — what a
  workgroup reads from the running prefix when the last L row blocks of its tree are still in flight;
  usable once rb - L >= --min-count blocks have finished, else the first-tile guess.

With two candidates the binades are those of g / sqrt 2 and the next; with one, g's own.  Exact half-ulp
ties (which poison a candidate) are not modelled.

  python tools/fold_cand_sim.py                                  # C2: 10k trees x 2^20 rows, every 14th complete tree
  python tools/fold_cand_sim.py --data test --rows 524288 --trees 1200 --seed 7 --block-rows 1024 --every 1
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "symbolicregression.jl_amd"), os.path.join(ROOT, "oracle"), ROOT]

OPS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])


def binade(x):
    return np.floor(np.log2(np.maximum(x, 1e-300)))


def data(kind, n):
    if kind == "bench":
        import bench
        return bench.c2_data(n, 0)
    rng = np.random.default_rng(2)  # (the GPU tests' dataset: tests/test_gpu_fold_compact.py)
    X = rng.standard_normal((5, n)).astype(np.float32)
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    return X, y


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", choices=["bench", "test"], default="bench")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--trees", type=int, default=10_000)
    ap.add_argument("--seed", type=int, default=1, help="population seed")
    ap.add_argument("--block-rows", type=int, default=2048, help="rows of a row block (C2: two 1,024-row tiles)")
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--every", type=int, default=14, help="simulate every k-th complete tree")
    ap.add_argument("--lag", type=int, nargs="+", default=[16, 32, 64, 128])
    ap.add_argument("--min-count", type=int, nargs="+", default=[8])
    ap.add_argument("--cands", type=int, nargs="+", default=[2, 1])
    ap.add_argument("--delta-log2", type=int, default=8)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()

    from oracle import Oracle
    from sr_amd import Options, flatten_trees, gen_random_population

    n, rbr, tile = args.rows, args.block_rows, args.tile
    assert n % rbr == 0 and rbr % tile == 0
    nb, tpb = n // rbr, rbr // tile
    X, y = data(args.data, n)
    opts = Options(**OPS)
    tb = flatten_trees(gen_random_population(args.trees, opts, 5, max_size=30, seed=args.seed), np.float32)
    orc = Oracle.from_options(opts)
    L, C = orc.eval_loss_batch(tb, X, y, accum="f64", n_threads=args.threads)
    idx = np.nonzero(C & np.isfinite(L))[0][::args.every]
    dd = 2.0 ** -args.delta_log2
    rb = np.arange(nb)
    keys = [("first tile", nc, 0, 0) for nc in args.cands]
    keys += [(f"prefix lag {lag} min {mc}", nc, lag, mc) for nc in args.cands for mc in args.min_count for lag in args.lag]
    left = {k: 0 for k in keys}
    slow_n = pairs = 0
    for k in idx:
        p, _ = orc.eval_tree_array(tb, int(k), X)
        d = (p - y).astype(np.float32)
        l = (d * d).astype(np.float64)
        segs = l.reshape(nb, rbr).sum(1)
        t0 = l.reshape(nb, tpb, tile)[:, 0, :].sum(1)
        Sb = np.concatenate([[0.0], np.cumsum(segs)])
        qa = binade(Sb[:-1] * (1 - dd))
        steps = qa == binade(Sb[1:] * (1 + dd))
        steps[0] = False
        pairs += nb
        slow_n += int((~steps).sum())
        first = rb * tpb * t0
        for key in keys:
            _, nc, lag, mc = key
            g = first
            if lag:
                done = rb - lag
                use = done >= mc
                est = Sb[np.maximum(done, 0)] * rb / np.maximum(done, 1)
                g = np.where(use, est, first)
            off = qa - binade(g * (0.7071067811865476 if nc == 2 else 1.0))
            hit = steps & (off >= 0) & (off < nc)
            left[key] += nb - int(hit.sum())
    print(f"{len(idx)} complete trees, {nb} row blocks of {rbr} rows ({tpb} tiles), delta 2^-{args.delta_log2}: "
          f"{pairs} (tree, block) pairs")
    print(f"| {'guess of the prefix at block rb':44s} | candidates | pairs left to the FOLD pass |")
    print(f"| {'none possible (the plan calls the block slow)':44s} | {'-':10s} | {100.0 * slow_n / pairs:6.2f} % |")
    for key in keys:
        print(f"| {key[0]:44s} | {key[1]:10d} | {100.0 * left[key] / pairs:6.2f} % |")


if __name__ == "__main__":
    main()
