"""RecVAE's two row-wise kernels and a training epoch beside the same numbers from torch's own operators on the same card. Four
measurements, each the package against the torch composition of the same definitions (``F.layer_norm``, ``sigmoid``, ``logsumexp``, ...):
  1. ``ops.SwishLayerNormFn`` forward plus backward at 500 x 600 (with the running sum on both sides);
  2. ``ops.CompositePriorKLFn`` forward plus backward at 500 x 200;
  3. one encoder pass and 4. one full epoch (3 encoder passes, the prior update, 1 decoder pass) of ``RecVAE`` at ML-1M's dimensions
     (6,040 x 3,706, synthetic interactions, batch 500, hidden 600, latent 200, dropout 0.5), against the same network in plain torch
     (dense input rows, nn.Linear, F.dropout, two torch.optim.Adam).
The two sides of 1 and 2 must agree (1e-4 relative to the largest magnitude), the step fails otherwise. Device-event times, one warm-up,
then the median of --reps runs. Prints one JSON line. Stand-alone: nothing is gated on these figures.

    python tools/time_recvae.py [--reps 7]
"""
import argparse
import copy
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_als import timed                      # noqa: E402

LOG2PI = math.log(2 * math.pi)
LOGW = (math.log(3 / 20), math.log(3 / 4), math.log(1 / 10))


def swish_ln_torch(a, r, gamma, beta):
    s = a + r
    h = F.layer_norm(s * torch.sigmoid(s), (a.shape[1],), gamma, beta, 0.1)
    return h, r + h


def log_normal(z, m, v):
    return -0.5 * (v + LOG2PI + (z - m) ** 2 / torch.exp(v))


def prior_kl_torch(mu, logvar, eps, mu_old, logvar_old, weight):
    z = mu + eps * torch.exp(0.5 * logvar)
    zero = torch.zeros_like(z)
    comps = torch.stack([LOGW[0] + log_normal(z, zero, zero), LOGW[1] + log_normal(z, mu_old, logvar_old), LOGW[2] + log_normal(z, zero, zero + 10.0)])
    return z, (weight * (log_normal(z, mu, logvar) - torch.logsumexp(comps, 0)).sum(1)).mean()


def agree(a, b, what):
    a, b = a.detach(), b.detach()
    scale = max(float(b.abs().max()), 1e-30)
    assert float((a - b).abs().max()) <= 1e-4 * scale, (what, float((a - b).abs().max()), scale)


def swish_ln_step(S, B, H, reps, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    a, r, dh, dr = (torch.randn(B, H, device=dev, generator=g) for _ in range(4))
    gamma, beta = 1 + 0.1 * torch.randn(H, device=dev, generator=g), torch.randn(H, device=dev, generator=g)

    def run(fn):
        leaves = [t.detach().clone().requires_grad_() for t in (a, r, gamma, beta)]
        h, ro = fn(*leaves)
        torch.autograd.backward([h, ro], [dh, dr])
        return [h, ro] + [t.grad for t in leaves]

    kernel = lambda: run(lambda *t: S.ops.SwishLayerNormFn.apply(*t, 0.1, True))       # noqa: E731
    composed = lambda: run(swish_ln_torch)                                             # noqa: E731
    for x, y, name in zip(kernel(), composed(), ('h', 'r_out', 'da', 'dr_in', 'dgamma', 'dbeta')):
        agree(x, y, name)
    return {'shape': [B, H], 'kernel_ms': timed(kernel, reps), 'torch_ms': timed(composed, reps)}


def prior_kl_step(S, B, L, reps, dev):
    g = torch.Generator(device=dev).manual_seed(2)
    mu, eps, mu_old, dz = (torch.randn(B, L, device=dev, generator=g) for _ in range(4))
    logvar, logvar_old = (torch.randn(B, L, device=dev, generator=g) - 1 for _ in range(2))
    weight = 0.005 * torch.randint(1, 300, (B,), device=dev, generator=g).float()

    def run(fn):
        m, lv = mu.detach().clone().requires_grad_(), logvar.detach().clone().requires_grad_()
        z, kl = fn(m, lv, eps, mu_old, logvar_old, weight)
        ((z * dz).sum() + kl).backward()
        return [z, kl, m.grad, lv.grad]

    kernel = lambda: run(S.ops.CompositePriorKLFn.apply)                               # noqa: E731
    composed = lambda: run(prior_kl_torch)                                             # noqa: E731
    for x, y, name in zip(kernel(), composed(), ('z', 'kl', 'dmu', 'dlogvar')):
        agree(x, y, name)
    return {'shape': [B, L], 'kernel_ms': timed(kernel, reps), 'torch_ms': timed(composed, reps)}


class TorchEncoder(torch.nn.Module):
    def __init__(self, n_items, hidden, latent):
        super().__init__()
        self.fc = torch.nn.ModuleList([torch.nn.Linear(n_items if k == 0 else hidden, hidden) for k in range(5)])
        self.ln = torch.nn.ModuleList([torch.nn.LayerNorm(hidden, eps=0.1) for _ in range(5)])
        self.mu, self.logvar = torch.nn.Linear(hidden, latent), torch.nn.Linear(hidden, latent)

    def forward(self, x, p):
        x = F.dropout(F.normalize(x), p, True) if p else F.normalize(x)
        hs = []
        for fc, ln in zip(self.fc, self.ln):
            pre = fc(x if not hs else hs[-1])
            for h in hs:
                pre = pre + h
            hs.append(ln(pre * torch.sigmoid(pre)))
        return self.mu(hs[-1]), self.logvar(hs[-1])


def epoch_step(S, datasets, reps, dev):
    m = datasets.synthetic_interactions(6040, 3706, 1000209, seed=3, item_popularity=1.0)
    model = S.RecVAE(n_epochs=0, device=dev).fit(m)             # the training state without an epoch
    enc, dec = TorchEncoder(3706, 600, 200).to(dev), torch.nn.Linear(200, 3706).to(dev)
    old = copy.deepcopy(enc)
    opt_e, opt_d = torch.optim.Adam(enc.parameters(), lr=5e-4), torch.optim.Adam(dec.parameters(), lr=5e-4)
    dense = torch.from_numpy(np.asarray(m.todense(), dtype=np.float32)).to(dev)
    active = torch.nonzero(dense.sum(1) > 0).reshape(-1)

    def torch_pass(encoder_pass):
        order = active[torch.randperm(active.numel(), device=dev)]
        for lo in range(0, order.numel(), 500):
            x = dense[order[lo:lo + 500]]
            with torch.set_grad_enabled(encoder_pass):
                mu, logvar = enc(x, 0.5 if encoder_pass else 0.0)
            with torch.no_grad():
                mu_old, logvar_old = old(x, 0.0)
            z, kl = prior_kl_torch(mu, logvar, torch.randn_like(mu), mu_old, logvar_old, 0.005 * x.sum(1))
            loss = (-(F.log_softmax(dec(z), 1) * x).sum(1)).mean() + kl
            opt = opt_e if encoder_pass else opt_d
            opt.zero_grad()
            loss.backward()
            opt.step()

    def torch_epoch():
        for _ in range(3):
            torch_pass(True)
        old.load_state_dict(enc.state_dict())
        torch_pass(False)

    return {'shape': [6040, 3706], 'nnz': int(m.nnz),
            'package_encoder_pass_ms': timed(lambda: model.train_pass('encoder'), reps), 'torch_encoder_pass_ms': timed(lambda: torch_pass(True), reps),
            'package_epoch_ms': timed(model.train_epoch, reps), 'torch_epoch_ms': timed(torch_epoch, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    import sibrar_amd as S
    from importlib import import_module
    datasets = import_module(S.ops.__name__.rsplit('.', 1)[0] + '.datasets')
    dev = torch.device('cuda:0')
    out = {'swish_ln': swish_ln_step(S, 500, 600, args.reps, dev), 'prior_kl': prior_kl_step(S, 500, 200, args.reps, dev),
           'epoch': epoch_step(S, datasets, args.reps, dev)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
