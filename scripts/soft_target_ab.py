"""A/B of the step prologue with mixing and of the classifier head with soft targets (run on the GPU box).

Times, alternately in one process at the VGG-small step's shape (batch 256 out of a device-resident
50 000 x 32 x 32 x 8 train split, fp32 and bf16): ``rk_gather_batch`` (plain), ``rk_gather_batch_aug`` (pad 4, flip
0.5) and ``rk_gather_batch_mix`` on top of the same augmentation, blending (lam 0.7) and copying a box (16 x 16 of
the 32 x 32 pixels).  And, fp32 at B 256, D 512, 16 class columns of which 10 real: ``rk_head_fwd_bwd`` against
``rk_head_fwd_bwd_soft`` (partner labels, lam 0.7, eps 0.1).  Each sample is one replay of a captured graph of
``--chain`` back-to-back launches of one variant, timed with device events; the graphs alternate, ``--rounds``
samples each after ``--warmup`` untimed ones.  Per launch: the median and the minimum over the samples.  Nothing is
gated: the blend reads two rows per output row, so it is expected to approach three row volumes where the plain
launch moves two; the figures are recorded under "micro" of the output file (other keys of the file are kept).

usage: python scripts/soft_target_ab.py [--out profiles/soft_target_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def time_graphs(launches, args):
    """{name: launch} -> {name_us_median, name_us_min}: one captured chain per variant, replayed alternately."""
    from rafiki_amd.ops.graphs import capture
    graphs = {}
    for name, launch in launches.items():
        launch()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture(g):
            for _ in range(args.chain):
                launch()
        torch.cuda.synchronize()
        graphs[name] = g
    times = {name: [] for name in launches}
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.warmup + args.rounds):
        for name in launches:
            beg.record()
            graphs[name].replay()
            end.record()
            end.synchronize()
            if r >= args.warmup:
                times[name].append(beg.elapsed_time(end) * 1e3 / args.chain)      # us per launch
    res = {'launches_each': args.rounds * args.chain}
    for name, t in times.items():
        res[name + '_us_median'] = round(statistics.median(t), 3)
        res[name + '_us_min'] = round(min(t), 3)
    return res


def prologues(dtype, args, dev):
    from rafiki_amd.ops import functional as F
    from rafiki_amd.ops.augment import AUG_STREAM
    n, B, chain = args.rows, args.batch, args.chain
    gen = torch.Generator(device=dev).manual_seed(0)
    data = torch.randn((n, 32, 32, 8), device=dev, generator=gen).to(dtype)
    labels = torch.randint(0, 10, (n,), device=dev, generator=gen, dtype=torch.int32)
    sched = torch.randint(0, n, (chain, B), device=dev, generator=gen)
    out_x = torch.empty((B, 32, 32, 8), device=dev, dtype=dtype)
    out_y = torch.empty((B,), device=dev, dtype=torch.int32)
    out_y2 = torch.empty((B,), device=dev, dtype=torch.int32)
    lam_out = torch.zeros(1, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    epoch = torch.full((1,), 3, dtype=torch.int32, device=dev)
    lam_table = torch.full((chain,), 0.7, device=dev)
    box_table = torch.tensor([8, 24, 8, 24], dtype=torch.int32, device=dev).repeat(chain, 1)
    aug = dict(pad=4, flip_p=0.5, seed=0, stream_id=AUG_STREAM, epoch=epoch)
    mix = dict(lam_table=lam_table, box_table=box_table, out_y2=out_y2, lam_out=lam_out)
    res = time_graphs({
        'plain': lambda: F.gather_batch(data, labels, sched, counter, out_x, out_y, done=done),
        'aug': lambda: F.gather_batch_aug(data, labels, sched, counter, out_x, out_y, done=done, **aug),
        'aug_blend': lambda: F.gather_batch_mix(data, labels, sched, counter, out_x, out_y, done=done, kind='mixup',
                                                **mix, **aug),
        'aug_box': lambda: F.gather_batch_mix(data, labels, sched, counter, out_x, out_y, done=done, kind='cutmix',
                                              **mix, **aug)}, args)
    for name in ('aug', 'aug_blend', 'aug_box'):
        res[name + '_over_plain'] = round(res[name + '_us_median'] / res['plain_us_median'], 3)
    return res


def heads(args, dev):
    from rafiki_amd.ops import f32 as S
    B, D, NC, ncls = args.batch, 512, 16, 10
    gen = torch.Generator(device=dev).manual_seed(1)
    z = torch.relu(torch.randn((B, D), device=dev, generator=gen))
    w = torch.randn((NC, D), device=dev, generator=gen) * D ** -0.5
    b = torch.zeros(NC, device=dev)
    y = torch.randint(0, ncls, (B,), device=dev, generator=gen, dtype=torch.int32)
    y2 = torch.randint(0, ncls, (B,), device=dev, generator=gen, dtype=torch.int32)
    lam = torch.full((1,), 0.7, device=dev)
    dlog, dz = torch.empty((B, NC), device=dev), torch.empty((B, D), device=dev)
    loss = torch.zeros(1, device=dev)
    corr, seen = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    kw = dict(dlogits=dlog, dz=dz, gated=True, loss_sum=loss, correct=corr, counted=seen)
    res = time_graphs({
        'hard': lambda: S.head_fwd_bwd(z, w, b, y, ncls, **kw),
        'soft': lambda: S.head_fwd_bwd_soft(z, w, b, y, ncls, labels2=y2, lam=lam, eps=0.1, **kw)}, args)
    res['extra_us_median'] = round(res['soft_us_median'] - res['hard_us_median'], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/soft_target_ab.json')
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--chain', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('soft_target_ab.py needs the GPU: a time taken elsewhere says nothing')
    dev = torch.device('cuda', 0)
    res = {'shape': '{} of {} x 32 x 32 x 8'.format(args.batch, args.rows), 'pad': 4, 'flip_p': 0.5, 'lam': 0.7,
           'box': [8, 24, 8, 24], 'chain': args.chain, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(dev)}
    for name, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        res[name] = prologues(dtype, args, dev)
    res['head_fp32'] = heads(args, dev)
    print(json.dumps(res))
    whole = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            whole = json.load(f)
    whole['micro'] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(whole, f, indent=1)
        f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
