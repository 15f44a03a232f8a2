"""``sbr_multinomial_nll_f32`` (``ops.MultinomialNLLFn``) and a Mult-VAE training epoch beside the same numbers from torch's own operators on
the same card. Three measurements:
  1. the loss with its gradient at 500 x 3,706 and 500 x 50,000: the kernel, in place (one launch), against the torch composition
     ``F.log_softmax`` times a dense 0/1 target matrix (built outside the timed region), row sum, mean, ``backward``; both must agree on
     the loss within 1e-5 relative and on the gradient within 1e-6, the step fails otherwise;
  2. the kernel's achieved bytes per second, counting one read and one write of the logit matrix, beside the float4 copy rate the
     microarchitecture notes measure for this card (6.29 TB/s);
  3. one training epoch of ``MultVAE`` at ML-1M's dimensions (6,040 x 3,706, synthetic interactions, batch 500, hidden 600, latent 200,
     dropout 0.5) against the same network in plain torch (dense input rows, nn.Linear layers, F.dropout, torch.optim.Adam).
Device-event times, one warm-up, then the median of --reps runs. Prints one JSON line. Stand-alone: nothing is gated on these figures.

    python tools/time_multvae.py [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_als import timed                      # noqa: E402

HBM_COPY_TBS = 6.29


def loss_step(S, features, B, n_items, reps, dev):
    import scipy.sparse as sp
    rng = np.random.default_rng(1)
    dense = (rng.random((B, n_items)) < 0.02).astype(np.float32)
    csr = features.DeviceCSR(sp.csr_matrix(dense)).to(dev)
    targets = torch.from_numpy(dense).to(dev)
    rows = torch.arange(B, device=dev)
    z0 = torch.randn(B, n_items, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    work = torch.empty_like(z0)

    def kernel():
        S.ops._multinomial_nll('time_multvae', csr, rows, work, 1.0 / B, True)

    def kernel_with_copy():                       # the in-place launch eats its input: the timed region restores it first
        work.copy_(z0)
        kernel()

    def copy_only():
        work.copy_(z0)

    def composed():
        z = z0.detach().requires_grad_()
        (-(F.log_softmax(z, 1) * targets).sum(1)).mean().backward()
        return z

    work.copy_(z0)
    row_loss, _, d = S.ops._multinomial_nll('time_multvae', csr, rows, work, 1.0 / B, True)
    z = composed()
    want = float((-(F.log_softmax(z0.double(), 1) * targets).sum(1)).mean())
    assert abs(float(row_loss.double().mean()) - want) <= 1e-5 * abs(want), (float(row_loss.mean()), want)
    assert float((d - z.grad).abs().max()) <= 1e-6, float((d - z.grad).abs().max())
    t_kernel = timed(kernel_with_copy, reps) - timed(copy_only, reps)
    t_torch = timed(composed, reps)
    return {'shape': [B, n_items], 'kernel_ms': t_kernel, 'torch_ms': t_torch, 'kernel_tb_per_s': 8.0 * B * n_items / (t_kernel * 1e-3) / 1e12,
            'of_hbm_copy_rate': 8.0 * B * n_items / (t_kernel * 1e-3) / 1e12 / HBM_COPY_TBS}


class TorchMultVAE(torch.nn.Module):
    def __init__(self, n_items, hidden, latent):
        super().__init__()
        self.latent = latent
        self.enc1, self.enc2 = torch.nn.Linear(n_items, hidden), torch.nn.Linear(hidden, 2 * latent)
        self.dec1, self.dec2 = torch.nn.Linear(latent, hidden), torch.nn.Linear(hidden, n_items)

    def forward(self, x, beta):
        h = F.dropout(F.normalize(x), 0.5, True)
        e = self.enc2(torch.tanh(self.enc1(h)))
        mu, logvar = e[:, :self.latent], e[:, self.latent:]
        z = mu + torch.randn_like(mu) * torch.exp(0.5 * logvar)
        logits = self.dec2(torch.tanh(self.dec1(z)))
        kl = 0.5 * (-logvar + torch.exp(logvar) + mu * mu - 1).sum(1).mean()
        return (-(F.log_softmax(logits, 1) * x).sum(1)).mean() + beta * kl


def epoch_step(S, datasets, reps, dev):
    m = datasets.synthetic_interactions(6040, 3706, 1000209, seed=3, item_popularity=1.0)
    model = S.MultVAE(n_epochs=0, device=dev).fit(m)             # the training state without an epoch

    def package_epoch():
        model.train_epoch()

    net = TorchMultVAE(3706, 600, 200).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    dense = torch.from_numpy(np.asarray(m.todense(), dtype=np.float32)).to(dev)
    active = torch.nonzero(dense.sum(1) > 0).reshape(-1)

    def torch_epoch():
        order = active[torch.randperm(active.numel(), device=dev)]
        for lo in range(0, order.numel(), 500):
            loss = net(dense[order[lo:lo + 500]], 0.1)
            opt.zero_grad()
            loss.backward()
            opt.step()

    return {'shape': [6040, 3706], 'nnz': int(m.nnz), 'package_epoch_ms': timed(package_epoch, reps), 'torch_epoch_ms': timed(torch_epoch, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    import sibrar_amd as S
    from importlib import import_module
    pkg = S.ops.__name__.rsplit('.', 1)[0]
    features, datasets = import_module(pkg + '.features'), import_module(pkg + '.datasets')
    dev = torch.device('cuda:0')
    out = {'loss': [loss_step(S, features, 500, n, args.reps, dev) for n in (3706, 50000)], 'epoch': epoch_step(S, datasets, args.reps, dev)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
