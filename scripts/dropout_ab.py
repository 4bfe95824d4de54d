"""A/B of dropout in the captured training step (run on the GPU box).

Kernel: ``rk_dropout`` per launch at the VGG-small step's three uses at batch 256 — the [256, 2048] features at rate
0.25, the [256, 512] hidden activation at rate 0.5 and the two gradients that arrive at them (the same launch on
another buffer) — in fp32 and bf16.  Each sample is one replay of a captured graph of ``--chain`` back-to-back
launches of one variant, timed with device events; the graphs alternate, ``--rounds`` samples each after
``--warmup`` untimed ones.  Per launch: the median and the minimum over the samples.

Step: the whole captured fp32 VGG-small step (scheduled graph, SGD, batch 256) with dropout 0.5 / feature dropout
0.25 and with both at 0, two engines in one process replayed alternately in chains of ``--step-chain``; and, with
``--parent DIR`` (a checkout of the parent commit with its libraries built), the parent's step measured the same
way in a process of its own, the two processes taking turns ``--turns`` times.  Per step: median and minimum.

Nothing is gated.  The figures go under "micro" and "step" of the output file (other keys of the file are kept).

usage: python scripts/dropout_ab.py [--parent DIR] [--out profiles/dropout_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_graphs(launches, args):
    """{name: launch} -> {name_us_median, name_us_min}: one captured chain per variant, replayed alternately."""
    import torch
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


def micro(dtype, args, dev):
    import torch
    from rafiki_amd.ops import functional as F
    from rafiki_amd.ops.dropout import DROP_STREAM
    B = args.batch
    gen = torch.Generator(device=dev).manual_seed(0)
    step = torch.full((1,), 7, dtype=torch.int32, device=dev)
    epoch = torch.full((1,), 3, dtype=torch.int32, device=dev)
    # repeated in-place launches scale the survivors by 1 / (1 - p) each time: the values overflow to inf along a
    # chain, which costs an elementwise kernel nothing
    bufs = {'features': (torch.relu(torch.randn((B, 2048), device=dev, generator=gen)).to(dtype), 0.25, 0),
            'hidden': (torch.relu(torch.randn((B, 512), device=dev, generator=gen)).to(dtype), 0.5, 1),
            'd_features': (torch.randn((B, 2048), device=dev, generator=gen).to(dtype), 0.25, 0),
            'd_hidden': (torch.randn((B, 512), device=dev, generator=gen).to(dtype), 0.5, 1)}
    return time_graphs({name: (lambda t=t, p=p, k=k: F.dropout_(t, p, seed=1, site=DROP_STREAM + k, step=step,
                                                                epoch=epoch))
                        for name, (t, p, k) in bufs.items()}, args)


def child(args):
    """One process: the engines of ``--variants`` (name:dropout:feature_dropout) replayed alternately."""
    sys.path.insert(0, args.repo)
    import torch
    from rafiki_amd.engine.convnet import ConvNetEngine
    dev = torch.device('cuda', 0)
    B, chain = args.batch, args.step_chain
    total = (args.warmup + args.rounds) * chain
    gen = torch.Generator(device=dev).manual_seed(0)
    engines = {}
    for spec in args.variants.split(','):
        name, p, fp = spec.split(':')
        kw = {k: float(v) for k, v in (('dropout', p), ('feature_dropout', fp)) if float(v) > 0.0}
        eng = ConvNetEngine(num_classes=10, in_channels=3, image_size=32, device=dev, seed=0, dtype='fp32', **kw)
        data = torch.randn((8192, 32, 32, eng.cin_p), device=dev, generator=gen)
        labels = torch.randint(0, 10, (8192,), device=dev, generator=gen, dtype=torch.int32)
        eng.capture_scheduled(data, labels, total, B)
        eng.set_schedule(torch.randint(0, 8192, (total, B), device=dev, generator=gen), epoch=0)
        engines[name] = eng
    times = {name: [] for name in engines}
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.warmup + args.rounds):
        for name, eng in engines.items():
            beg.record()
            for _ in range(chain):
                eng.replay()
            end.record()
            end.synchronize()
            if r >= args.warmup:
                times[name].append(beg.elapsed_time(end) / chain)      # ms per step
    print('DROPOUT_AB ' + json.dumps(times))
    return 0


def steps(args):
    """Alternate a process of this tree (drop, zero) with one of the parent's tree (parent), pool the samples."""
    pooled = {}
    plan = [(HERE, 'drop:0.5:0.25,zero:0:0')] + ([(os.path.abspath(args.parent), 'parent:0:0')] if args.parent else [])
    for _ in range(args.turns):
        for repo, variants in plan:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--repo', repo, '--variants', variants,
                   '--batch', str(args.batch), '--step-chain', str(args.step_chain), '--rounds', str(args.rounds),
                   '--warmup', str(args.warmup)]
            out = subprocess.run(cmd, cwd=repo, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit('child failed ({}):\n{}'.format(out.returncode, out.stderr[-2000:]))
            line = [l for l in out.stdout.splitlines() if l.startswith('DROPOUT_AB ')][-1]
            for name, t in json.loads(line[len('DROPOUT_AB '):]).items():
                pooled.setdefault(name, []).extend(t)
    res = {'steps_each': args.turns * args.rounds * args.step_chain, 'turns': args.turns}
    for name, t in pooled.items():
        res[name + '_ms_median'] = round(statistics.median(t), 4)
        res[name + '_ms_min'] = round(min(t), 4)
    for name in ('zero', 'parent'):
        if name + '_ms_median' in res:
            res['drop_minus_' + name + '_us_median'] = round(1e3 * (res['drop_ms_median'] - res[name + '_ms_median']), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/dropout_ab.json')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--chain', type=int, default=100)
    ap.add_argument('--step-chain', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--turns', type=int, default=2)
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its libraries built')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--repo', default=HERE, help=argparse.SUPPRESS)
    ap.add_argument('--variants', default='', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('dropout_ab.py needs the GPU: a time taken elsewhere says nothing')
    step = steps(args)            # the children first: this process has not opened the GPU yet
    step.update(shape='VGG-small fp32, batch {}'.format(args.batch), chain=args.step_chain, rounds=args.rounds)
    print(json.dumps(step))
    dev = torch.device('cuda', 0)
    res = {'shape': '[{0}, 2048] at 0.25 and [{0}, 512] at 0.5'.format(args.batch), 'chain': args.chain,
           'rounds': args.rounds, 'device': torch.cuda.get_device_name(dev)}
    for name, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        res[name] = micro(dtype, args, dev)
    print(json.dumps(res))
    whole = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            whole = json.load(f)
    whole['micro'], whole['step'] = res, step
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(whole, f, indent=1)
        f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
