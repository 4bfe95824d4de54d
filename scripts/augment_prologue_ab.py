"""A/B of the step prologue with and without augmentation (run on the GPU box).

Times ``rk_gather_batch`` (the yardstick, unchanged) and ``rk_gather_batch_aug`` (pad 4, flip 0.5) alternately in
one process at the VGG-small step's shape: batch 256 out of a device-resident 50 000 x 32 x 32 x 8 train split,
fp32 and bf16.  Each sample is one replay of a captured graph of ``--chain`` back-to-back launches of one of the
two (the ``done`` counter walks a schedule of random rows, as in the training graph), timed with device events;
the two graphs alternate, ``--rounds`` samples each after ``--warmup`` untimed ones.  Per launch: the median and
the minimum over the samples.  The augmenting launch may cost at most 1 % of the VGG-small step (README) more
than the plain one; the script exits non-zero if it does not.

usage: python scripts/augment_prologue_ab.py [--out profiles/augment_prologue_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

STEP_MS = 1.84          # the VGG-small training step (README, fp32, batch 256)
BOUND_US = 0.01 * STEP_MS * 1e3


def measure(dtype, args, dev):
    from rafiki_amd.ops import functional as F
    from rafiki_amd.ops.augment import AUG_STREAM
    from rafiki_amd.ops.graphs import capture
    n, B, chain = args.rows, args.batch, args.chain
    gen = torch.Generator(device=dev).manual_seed(0)
    data = torch.randn((n, 32, 32, 8), device=dev, generator=gen).to(dtype)
    labels = torch.randint(0, 10, (n,), device=dev, generator=gen, dtype=torch.int32)
    sched = torch.randint(0, n, (chain, B), device=dev, generator=gen)
    out_x = torch.empty((B, 32, 32, 8), device=dev, dtype=dtype)
    out_y = torch.empty((B,), device=dev, dtype=torch.int32)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    epoch = torch.full((1,), 3, dtype=torch.int32, device=dev)

    def plain():
        F.gather_batch(data, labels, sched, counter, out_x, out_y, done=done)

    def aug():
        F.gather_batch_aug(data, labels, sched, counter, out_x, out_y, done=done, pad=4, flip_p=0.5, seed=0,
                           stream_id=AUG_STREAM, epoch=epoch)

    graphs = {}
    for name, launch in (('plain', plain), ('aug', aug)):
        launch()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture(g):
            for _ in range(chain):
                launch()
        torch.cuda.synchronize()
        graphs[name] = g
    times = {'plain': [], 'aug': []}
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.warmup + args.rounds):
        for name in ('plain', 'aug'):
            beg.record()
            graphs[name].replay()
            end.record()
            end.synchronize()
            if r >= args.warmup:
                times[name].append(beg.elapsed_time(end) * 1e3 / chain)      # us per launch
    res = {'launches_each': args.rounds * chain}
    for name, t in times.items():
        res[name + '_us_median'] = round(statistics.median(t), 3)
        res[name + '_us_min'] = round(min(t), 3)
    res['extra_us_median'] = round(res['aug_us_median'] - res['plain_us_median'], 3)
    res['extra_us_min'] = round(res['aug_us_min'] - res['plain_us_min'], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/augment_prologue_ab.json')
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--chain', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('augment_prologue_ab.py needs the GPU: a time taken elsewhere says nothing')
    dev = torch.device('cuda', 0)
    res = {'shape': '{} of {} x 32 x 32 x 8'.format(args.batch, args.rows), 'pad': 4, 'flip_p': 0.5,
           'chain': args.chain, 'rounds': args.rounds, 'step_ms': STEP_MS, 'bound_us': round(BOUND_US, 2),
           'device': torch.cuda.get_device_name(dev)}
    for name, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        res[name] = measure(dtype, args, dev)
    res['within_bound'] = all(res[k]['extra_us_median'] <= BOUND_US for k in ('fp32', 'bf16'))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    return 0 if res['within_bound'] else 1


if __name__ == '__main__':
    sys.exit(main())
