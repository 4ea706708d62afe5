"""Time of the point-set distance gradients against their forward kernels, on one device:
    dg_emd_grad          against dg_emd (paired)      32 pairs of 2048 x 2048 points, 4096 pairs of 512 x 512
    dg_chamfer_backward  against ONE dg_chamfer_nn    32 pairs of 65 536 points
    python scripts/bench_point_distance_grad.py [--rounds 7] [--window-ms 200]
Per shape the two kernels alternate: `warm` untimed rounds, then `rounds` rounds in which each kernel is launched back to
back for about --window-ms between two device events (the launch count per window is fixed after the warm-up from one timed
launch); the figure is the window's time per launch, reported as median and minimum over the rounds.  Before the timing the
outputs are checked at the timed size: dg_emd_grad's cost equals dg_emd's bit for bit, two gradient launches agree bit for
bit.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def alternate(fns, rounds, window_ms, warm=2):
    """{name: [ms per launch, one per round]} of the kernels in `fns`, alternating"""
    for _ in range(warm):
        for _, fn in fns:
            timed(fn, 1)
    count = {name: max(1, min(1000, int(window_ms / max(timed(fn, 1), 1e-3)))) for name, fn in fns}
    times = {name: [] for name, _ in fns}
    for _ in range(rounds):
        for name, fn in fns:
            times[name].append(timed(fn, count[name]))
    return times, count


def report(what, shape, times, count, base, new, extra=None):
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = {"what": what, **shape, "ms": {k: round(v, 4) for k, v in med.items()},
           "min_ms": {k: round(min(v), 4) for k, v in times.items()}, "max_ms": {k: round(max(v), 4) for k, v in times.items()},
           "launches_per_window": count, "ratio": round(med[new] / med[base], 3)}
    out.update(extra or {})
    print(json.dumps(out), flush=True)


def bench_emd(B, n, m, rounds, window_ms):
    from dusty_gan_amd import _lib as L
    lib = L.lib()
    gen = torch.Generator(device="cuda").manual_seed(n + B)
    a = torch.rand(B, n, 3, device="cuda", generator=gen) * 2 - 1
    b = (torch.rand(B, m, 3, device="cuda", generator=gen) * 2 - 1) * 0.9
    cost, cost_g = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    g1, g2 = torch.empty_like(a), torch.empty_like(b)

    def fwd():
        L.check(lib.dg_emd(L.ptr(a), B, n, L.ptr(b), B, m, 1, L.ptr(cost), L.stream_ptr()), "dg_emd")

    def grad():
        L.check(lib.dg_emd_grad(L.ptr(a), n, L.ptr(b), m, B, None, L.ptr(cost_g), L.ptr(g1), L.ptr(g2), L.stream_ptr()),
                "dg_emd_grad")

    fwd(), grad()
    h1, h2 = g1.clone(), g2.clone()
    grad()
    torch.cuda.synchronize()
    assert torch.equal(cost, cost_g) and torch.equal(h1, g1) and torch.equal(h2, g2) and bool(torch.isfinite(g1).all())
    times, count = alternate((("dg_emd", fwd), ("dg_emd_grad", grad)), rounds, window_ms)
    # per level dg_emd evaluates the n x m distances and exponentials three times, dg_emd_grad four times
    pairs = 10.0 * B * n * m
    med = sorted(times["dg_emd_grad"])[len(times["dg_emd_grad"]) // 2]
    report("EMD gradient against the cost alone", {"B": B, "n": n, "m": m}, times, count, "dg_emd", "dg_emd_grad",
           {"sweeps": {"dg_emd": 3, "dg_emd_grad": 4}, "grad_pair_evals_per_s": round(4.0 * pairs / (med * 1e-3), 0)})


def bench_chamfer(B, n, rounds, window_ms):
    from dusty_gan_amd import _lib as L
    lib = L.lib()
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = torch.rand(B, n, 3, device="cuda", generator=gen)
    b = torch.rand(B, n, 3, device="cuda", generator=gen)
    d1, d2 = torch.empty(B, n, device="cuda"), torch.empty(B, n, device="cuda")
    i1, i2 = (torch.empty(B, n, dtype=torch.int32, device="cuda") for _ in range(2))
    gd = torch.full((B, n), 1.0 / n, device="cuda")
    g1, g2 = torch.empty_like(a), torch.empty_like(b)
    acc = torch.zeros(B * 2 * n * 4, dtype=torch.int64, device="cuda")

    def nn(x, y, d, i):
        L.check(lib.dg_chamfer_nn(L.ptr(x), 3 * n, 3, 1, n, L.ptr(y), 3 * n, 3, 1, n, B, L.ptr(d), L.ptr(i), L.stream_ptr()),
                "dg_chamfer_nn")

    def bwd():
        L.check(lib.dg_chamfer_backward(L.ptr(a), n, L.ptr(b), n, B, L.ptr(gd), L.ptr(gd), L.ptr(i1), L.ptr(i2), L.ptr(g1),
                                        L.ptr(g2), L.ptr(acc), L.stream_ptr()), "dg_chamfer_backward")

    nn(a, b, d1, i1), nn(b, a, d2, i2), bwd()
    h1, h2 = g1.clone(), g2.clone()
    bwd()
    torch.cuda.synchronize()
    assert torch.equal(h1, g1) and torch.equal(h2, g2) and not bool(acc.any()) and bool(torch.isfinite(g1).all())
    times, count = alternate((("dg_chamfer_nn", lambda: nn(a, b, d1, i1)), ("dg_chamfer_backward", bwd)), rounds, window_ms)
    med = sorted(times["dg_chamfer_backward"])[len(times["dg_chamfer_backward"]) // 2]
    # algorithmic traffic of the backward per point: the point, its neighbour, g, idx (32 B), the direct term written and read
    # back (24 B), the gradient (12 B), the four scatter words read and re-zeroed (64 B) and three 8-byte atomic adds (24 B)
    report("Chamfer backward against one nearest-neighbour search", {"B": B, "n": n, "m": n}, times, count, "dg_chamfer_nn",
           "dg_chamfer_backward", {"backward_gb_per_s": round(156.0 * 2 * B * n / (med * 1e-3) / 1e9, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--tiny", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_distance_grad.py needs the GPU: nothing is measured without one")
    if args.tiny:
        bench_emd(4, 128, 128, 2, 5.0), bench_chamfer(2, 4096, 2, 5.0)
        return
    bench_emd(32, 2048, 2048, args.rounds, args.window_ms)
    bench_emd(4096, 512, 512, args.rounds, args.window_ms)
    bench_chamfer(32, 65536, args.rounds, args.window_ms)


if __name__ == "__main__":
    main()
