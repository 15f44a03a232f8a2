"""Cost of the deterministic mode: ms per step of c2 (B = 8192, B = 256) and c1 (B = 256) with the mode off and on, in one process,
through bench.py's own step construction (``bench.build`` / ``bench.bench_training``: same loader pipeline, warm-up, settle steps and
timed region as the bench line). Prints one JSON line; DESIGN.md section 9 quotes it.

    python tools/bench_deterministic.py [--steps 300] [--warmup 5] [--rounds 2]

Each configuration is timed ``--rounds`` times per mode, alternating off / on, so that clock drift of the box lands on both."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    args = ap.parse_args()
    import bench
    import sibrar_amd as S
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    out = {}

    def time_both(name, ds, net, batch, loss=None):
        sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
        res = {'off': [], 'on': []}
        for _ in range(args.rounds):
            for mode in ('off', 'on'):
                S.ops.set_deterministic(mode == 'on')
                S.ops.nondeterministic_launches(reset=True)
                net.load_state_dict(sd0)
                dt, _ = bench.bench_training(S, ds, net, dev, batch, args.steps, args.warmup, 0, 1, time_kernels=False, loss=loss)
                res[mode].append(round(dt / args.steps * 1e3, 4))
                if mode == 'on':
                    assert S.ops.nondeterministic_launches() == 0, f'{name}: arrival-order launches in deterministic mode'
        S.ops.set_deterministic(False)
        res['ratio'] = round(min(res['on']) / min(res['off']), 3)
        out[name] = res

    ds, net = bench.build(S, dict(bench.C2), dev)
    time_both('c2_b8192', ds, net, 8192)
    time_both('c2_b256', ds, net, 256)
    del ds, net
    C1 = bench.C1
    ds = S.SyntheticDataset(C1['n_users'], C1['n_items'], C1['nnz'], item_dense={'text': 768}, item_tags={'genres': (18, 3)}, seed=0,
                            n_negative_samples=C1['n_neg'], negative_sampling_strategy='uniform_recbole', holdout_per_user=1,
                            item_popularity=1.0)
    torch.manual_seed(42)
    np.random.seed(42)
    net = S.SingleBranchNet(S.SingleBranchNetConfig.from_dict(bench.C1_MODEL), ds).to(dev)
    bpr = S.RecBayesianPersonalizedRankingLoss(n_items=ds.n_items, aggregator='mean', train_neg_strategy='uniform_recbole',
                                               neg_train=ds.n_negative_samples)
    time_both('c1_b256', ds, net, 256, loss=bpr)
    print(json.dumps({'ms_per_step': out, 'steps': args.steps, 'warmup': args.warmup}))


if __name__ == '__main__':
    main()
