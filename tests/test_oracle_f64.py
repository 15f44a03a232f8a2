"""CPU: the oracle's float64 mode against the golden vectors of the real reference.

``oracle/model_ref.py`` computes in the dtype of the state dict it is given. The GPU tests use a float64 copy of a state dict
as *truth*; this pins that copy to the reference transitively: on every G4 case (lookup / linear / entity user sides x the five
rec losses) the float64 oracle reproduces the reference's fp32 loss and every gradient within fp32 rounding.
"""
import pytest
import torch

from golden_util import MANIFEST, load, state_dict, sub, world, ref_tables, close, gscale, bn_shadowed_biases, I
from oracle import model_ref, losses_ref

from test_oracle_golden import _LOSS, _orders


def _widened(z, prefix):
    """The golden state dict with every floating-point tensor widened to float64 (exact), trainables requiring grad."""
    sd = {}
    for k, v in state_dict(z, prefix).items():
        if v.dtype.is_floating_point:
            v = v.double()
            if 'running_' not in k:
                v.requires_grad_(True)
        sd[k] = v
    return sd


@pytest.mark.parametrize('case', MANIFEST['g4_full_net']['cases'], ids=lambda c: c['name'])
def test_g4_full_net_in_float64(case):
    z = load('g4_full_net')
    n = case['name']
    sd = _widened(z, f'{n}/sd0/')
    assert model_ref.float_dtype(sd) == torch.float64
    ut, it = ref_tables(world(z))
    cfg = {'shared_common_dim': case['shared_common_dim'], 'user': case['user'], 'item': case['item']}
    net = model_ref.RefSingleBranchNet(sd, cfg, ut, it, orders=_orders(case))
    u, i, labels = (torch.from_numpy(z[f'{n}/{k}']) for k in ('u', 'i', 'labels'))
    um = z[f'{n}/user_mods'] if f'{n}/user_mods' in z.files else None
    logits = net.forward(u, i, True, um, z[f'{n}/item_mods'])
    assert logits.dtype == torch.float64
    close(logits, z[f'{n}/logits'], what='logits', rtol=1e-5, norm_rtol=1e-5)
    loss = losses_ref.RefRecLoss(n_items=I, neg_train=3, **_LOSS[case['loss']]).compute_loss(logits, labels)
    assert loss.dtype == torch.float64
    close(loss, z[f'{n}/rec_loss'], what='rec_loss', rtol=1e-5, norm_rtol=1e-5)
    reg = net.get_and_reset_other_loss()
    assert reg['reg_loss'].dtype == torch.float64
    close(reg['reg_loss'], z[f'{n}/reg_loss'], what='reg_loss', rtol=1e-5, norm_rtol=1e-5)
    (loss + reg['reg_loss']).backward()
    gs = sub(z, f'{n}/g/')
    # a bias in front of a BatchNorm has a zero gradient by maths: the golden value is the reference's fp32 rounding noise, bounded
    # at the scale of the gradients it is a sum of (the float64 oracle returns ~1e-17 there)
    shadowed = bn_shadowed_biases(sd.keys())
    for k, g in gs.items():
        got = sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])
        assert got.dtype == torch.float64, k
        close(got, g, what=f'g/{k}', rtol=1e-5, norm_rtol=1e-5, scale=gscale(gs.values()) if k in shadowed else 0.)
    # the BatchNorm running statistics the forward pass updated, in float64, against the reference's after its step
    sd1 = sub(z, f'{n}/sd1/')
    for k, v in sd.items():
        if 'running_' in k:
            assert v.dtype == torch.float64, k
            close(v, sd1[k], what=f'sd1/{k}', rtol=1e-5, norm_rtol=1e-5)
        elif 'num_batches_tracked' in k:
            assert int(v) == int(sd1[k]), k
