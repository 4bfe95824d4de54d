"""A/B of global-norm gradient clipping in the captured training step (run on the GPU box).

Kernel: ``rk_grad_sumsq`` alone over a gradient arena of the VGG-small size, as a captured chain of ``--chain``
back-to-back launches timed with device events, ``--rounds`` samples after ``--warmup`` untimed ones: the median and
the minimum per launch, next to the time its bytes (4 per element) take at the HBM rates of the architecture notes.

Step: the whole captured fp32 VGG-small step (scheduled graph, SGD, batch 256), replayed in chains of
``--step-chain``.  What clipping costs: ``clip_norm`` off, inf (measure only) and 1.0 as three engines of one
process replayed alternately (``off_alt``, ``inf``, ``on``).  What the feature costs when off: one engine with
``clip_norm`` off alone in a process (``off``) and, with ``--parent DIR`` (a checkout of the parent commit with its
libraries built), the parent's engine alone in a process of its tree (``parent``) — the same conditions for both.
The processes take turns ``--turns`` times.  Per step: the median and the minimum over all samples, and the median
of each turn — the spread of those turn medians is the run-to-run spread that the off-minus-parent difference is
read against.

Nothing is gated.  The figures go under "micro" and "step" of the output file (other keys of the file are kept).

usage: python scripts/grad_clip_ab.py [--parent DIR] [--out profiles/grad_clip_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12     # bytes / s: the spec rate and the measured float4-copy rate


def micro(args, dev, numel):
    import torch
    from rafiki_amd.ops import functional as F
    from rafiki_amd.ops.graphs import capture
    g = torch.randn(numel, device=dev)
    part = torch.zeros(F.sumsq_parts(numel), dtype=torch.float64, device=dev)
    F.grad_sumsq(g, part)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture(graph):
        for _ in range(args.chain):
            F.grad_sumsq(g, part)
    torch.cuda.synchronize()
    times = []
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.warmup + args.rounds):
        beg.record()
        graph.replay()
        end.record()
        end.synchronize()
        if r >= args.warmup:
            times.append(beg.elapsed_time(end) * 1e3 / args.chain)      # us per launch
    return {'numel': numel, 'partials': part.numel(), 'bytes': 4 * numel, 'chain': args.chain, 'rounds': args.rounds,
            'reduce_us_median': round(statistics.median(times), 3), 'reduce_us_min': round(min(times), 3),
            'hbm_peak_us': round(4 * numel / HBM_PEAK * 1e6, 3), 'hbm_copy_rate_us': round(4 * numel / HBM_COPY * 1e6, 3),
            'device': torch.cuda.get_device_name(dev)}


def child(args):
    """One process: the engines of ``--variants`` (name:clip_norm, ``-`` for none) replayed alternately."""
    sys.path.insert(0, args.repo)
    import torch
    from rafiki_amd.engine.convnet import ConvNetEngine
    dev = torch.device('cuda', 0)
    B, chain = args.batch, args.step_chain
    total = (args.warmup + args.rounds) * chain
    gen = torch.Generator(device=dev).manual_seed(0)
    engines = {}
    for spec in args.variants.split(','):
        name, clip = spec.split(':')
        kw = {} if clip == '-' else {'clip_norm': float(clip)}
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
    stats = {name: eng.grad_stats() for name, eng in engines.items() if getattr(eng, 'clip_norm', None) is not None}
    print('GRAD_CLIP_AB ' + json.dumps({'times': times, 'stats': stats,
                                        'numel': next(iter(engines.values())).flat.total}))
    return 0


def steps(args):
    """Processes in turn: this tree's off engine alone, the parent's alone, this tree's off / inf / on together."""
    pooled, turns, info = {}, {}, {}
    plan = [(HERE, 'off:-')] + ([(os.path.abspath(args.parent), 'parent:-')] if args.parent else []) + \
        [(HERE, 'off_alt:-,inf:inf,on:1.0')]
    for _ in range(args.turns):
        for repo, variants in plan:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--repo', repo, '--variants', variants,
                   '--batch', str(args.batch), '--step-chain', str(args.step_chain), '--rounds', str(args.rounds),
                   '--warmup', str(args.warmup)]
            out = subprocess.run(cmd, cwd=repo, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit('child failed ({}):\n{}'.format(out.returncode, out.stderr[-2000:]))
            line = [l for l in out.stdout.splitlines() if l.startswith('GRAD_CLIP_AB ')][-1]
            got = json.loads(line[len('GRAD_CLIP_AB '):])
            for name, t in got['times'].items():
                pooled.setdefault(name, []).extend(t)
                turns.setdefault(name, []).append(round(statistics.median(t), 4))
            info['numel'] = got['numel']
            info.setdefault('grad_stats', {}).update(got['stats'])
    res = {'steps_each': args.turns * args.rounds * args.step_chain, 'turns': args.turns, 'arena_numel': info['numel'],
           'grad_stats_last_turn': info['grad_stats']}
    for name, t in pooled.items():
        res[name + '_ms_median'] = round(statistics.median(t), 4)
        res[name + '_ms_min'] = round(min(t), 4)
        res[name + '_ms_turn_medians'] = turns[name]
    res['turn_spread_us'] = round(1e3 * max(max(v) - min(v) for v in turns.values()), 2)
    for name in ('inf', 'on'):
        res[name + '_minus_off_alt_us_median'] = round(1e3 * (res[name + '_ms_median'] - res['off_alt_ms_median']), 2)
    if 'parent_ms_median' in res:
        res['off_minus_parent_us_median'] = round(1e3 * (res['off_ms_median'] - res['parent_ms_median']), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/grad_clip_ab.json')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--chain', type=int, default=100)
    ap.add_argument('--step-chain', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--turns', type=int, default=3)
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
        raise SystemExit('grad_clip_ab.py needs the GPU: a time taken elsewhere says nothing')
    step = steps(args)            # the children first: this process has not opened the GPU yet
    step.update(shape='VGG-small fp32, batch {}'.format(args.batch), chain=args.step_chain, rounds=args.rounds)
    print(json.dumps(step))
    res = micro(args, torch.device('cuda', 0), step['arena_numel'])
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
