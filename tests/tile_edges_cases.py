"""What tests/test_hip_tile_edges.py and tests/test_tile_edges_cpu.py share — a test helper, not a test: the covering list of shapes of the
kernels on the 64 x 64 fp32 tile skeleton (csrc/tile64_f32.h), their inputs, the float64 / fp32 CPU references of every output AND every
saved tensor of the raw entry points, the preconditions that keep the discrete decisions (arg-mins, top-k masks, clamps, ReLU gates)
well-posed, and a Python restatement of the host-side launch rules. Everything here runs on the CPU.

Shapes. (R, D, N) sits on the edges of the tile (64), of the K-chunk (32) and of the register-block count NPT = ceil(N / 64):
R in {1, 63, 64, 65, 129}, D in {1, 31, 32, 33, 64, 65, 512}, N in {2, 63, 64, 65, 129, 192, 193, 256} as a covering list (BASE), plus the
reach shapes below, each derived from the restated rules (and asserted against them in tests/test_tile_edges_cpu.py)."""
import functools

import torch
from torch.nn import functional as F

import acf_ref
import ecf_ref
import protomf_inputs
import protomf_ref
import protomfs_ref
import sibrar_amd
from test_hip_acf import KAPPA, REL_FLOOR, W_EXC, W_INC, _with_threads                # noqa: F401  (re-exported)
from test_hip_ecf import NEAR_TIE, NEAR_TIE_CAP, TEMP                                 # noqa: F401
from test_hip_protomf import W_PROTO, W_BATCH

EPS = 1e-12                       # F.normalize's eps (T64_EPS)
KINK = 1e-3                       # tests/test_hip_protomfs.py: distance of every |cos| from the clamp, of every non-zero weight from 0

# ---- the host-side rules, restated -------------------------------------------------------------------------------------------------------
T64_T, T64_MAX_WG = sibrar_amd.ops.ANCHOR_TILE, sibrar_amd.ops.ANCHOR_MAX_WG          # 64, 1024: mirrored in ops.py
T64_WS_FLOATS, T64_MIN_SPLIT = 16 << 20, 64                                           # csrc/tile64_f32.h
PS_MAX_WG, PC_MAX_WG, PC_MAX_SPLIT = 256, 8192, 256                                   # csrc/proto_cos.hip
T64_MAX_N = 256


def tiles(n):
    return (n + T64_T - 1) // T64_T


def t64_wgs(R, max_wg=T64_MAX_WG):
    """workgroups of a pass over R rows; a workgroup walks the tiles blockIdx.x, blockIdx.x + wgs, ..."""
    return min(tiles(R), max_wg)


def t64_splits(R, part_floats):
    return min(min(max(T64_WS_FLOATS // part_floats, T64_MIN_SPLIT), T64_MAX_WG), tiles(R))


def pc_splits(R, D, N):
    """proto_cos.hip's dP pass: split s takes the ceil(tiles / splits) consecutive tiles from s * that on"""
    return max(min(PC_MAX_SPLIT // (tiles(D) * tiles(N)), tiles(R)), 1)


def am_splits(R, D, K):
    return t64_splits(R, D * K)


def ca_splits(R, D, C):
    return t64_splits(R, (D + 1) * C)


def ws_bytes(entry, R, D, N, backward):
    """the byte counts of the three ``*_workspace`` entry points, from the comments above their ``*_ws_bytes`` functions"""
    if entry == 'sbr_proto_sim_workspace' and not backward:
        wg = t64_wgs(R, PS_MAX_WG)
        return wg * 8 + 2 * T64_MAX_N * 4 + wg * N * 8
    if entry == 'sbr_proto_score_workspace' and not backward:
        return 2 * T64_MAX_N * 4
    if entry in ('sbr_proto_sim_workspace', 'sbr_proto_score_workspace'):
        return pc_splits(R, D, N) * N * (D + 1) * 4
    if entry == 'sbr_anchor_mix_workspace':
        return am_splits(R, D, N) * N * D * 4 if backward else t64_wgs(R) * (N + 1) * 8
    assert entry == 'sbr_cluster_affil_workspace'
    return 2 * T64_MAX_N * 4 + (ca_splits(R, D, N) * N * (D + 1) * 4 if backward else 0)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
BASE = [(1, 1, 2), (63, 31, 63), (64, 32, 64), (65, 33, 65), (129, 65, 129), (65, 64, 192), (64, 33, 193), (65, 5, 256), (129, 512, 2)]
REACH_FWD = (65601, 5, 3)
"""forward only. 1026 row tiles, the last of one row. anchor_mix and cluster_affil launch T64_MAX_WG = 1024 workgroups, so workgroups 0
and 1 walk a second tile; ProtoMF's forward launches PS_MAX_WG = 256, so every workgroup walks four or five."""
REACH_FWD_SCORE = (PC_MAX_WG * T64_T + 1, 5, 3)
"""forward only, sbr_proto_score_fwd: its grid cap is PC_MAX_WG = 8192 workgroups, so the loop needs 8193 tiles = 524,289 rows (the last
tile of one row); at D = 5, N = 3 that is 10 MB of table."""
REACH_BWD = (8257, 512, 256)
"""130 row tiles, the last of one row, at the largest partial (D N = 2^17 floats): anchor_mix has 128 splits and cluster_affil 127
((D + 1) N floats per partial), so their workgroups 0, 1 (and 2) own a second tile: the `first == false` arm of t64_part_add and the
`+=` of the column sums. proto_cos.hip splits by pc_splits (8 splits of 17 tiles here), which the large shapes of its own tests reach too."""

_ALT = [True, False]
SIM_CASES = [(R, D, N, (R, D, N) not in ((64, 32, 64), (65, 5, 256)), False) for R, D, N in BASE] + [REACH_FWD + (True, True), REACH_BWD + (True, False)]
"""(R, D, P, lookup, forward only); lookup False: rows == NULL"""
_FORMS = [(1, True), (3, False), (3, True), (1, False)]
SCORE_CASES = ([(R, D, N, 0, False, _ALT[n % 2], False) for n, (R, D, N) in enumerate(BASE)]
               + [(R, D, N) + _FORMS[n % 4] + (_ALT[(n // 2) % 2], False) for n, (R, D, N) in enumerate(BASE)]
               + [REACH_FWD_SCORE + (0, False, True, True), REACH_FWD + (3, True, True, True), REACH_BWD + (3, True, True, False)])
"""(R, D, P, fan, widx given, lookup, forward only); fan 0: the cosine form (Wt == NULL)"""
ANCHOR_CASES = ([(R, D, N, True, _ALT[n % 2], False) for n, (R, D, N) in enumerate(BASE)]
                + [(R, D, N, False, True, False) for R, D, N in ((63, 31, 63), (65, 33, 65), (65, 64, 192), (64, 33, 193))]
                + [REACH_FWD + (True, True, True), REACH_BWD + (True, True, False)])
"""(R, D, K, with the loss outputs, lookup, forward only)"""
_TOPS = [2, 1, 32, 65, 20, 96, 193, 100, 1]                       # 1, a middle value and C each at several NPT
CLUSTER_CASES = [(R, D, N, top, False) for (R, D, N), top in zip(BASE, _TOPS)] + [REACH_FWD + (2, True), REACH_BWD + (20, False)]
"""(R, D, C, top, forward only), run in the cosine and in the logit form"""
OPS_SHAPES = [(65, 33, 65), (129, 65, 129)]                       # the autograd functions on a column slice of a wider tensor


def case_id(c):
    return '-'.join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def _dups(idx):
    """a permutation with two duplicates, where there is room"""
    if len(idx) >= 4:
        idx[-1], idx[len(idx) // 2] = idx[0], idx[1]
    return idx.to(torch.int32)


def lowest_arg(dis, dim):
    """arg-min with the kernels' tie rule: the lowest index"""
    return (dis == dis.min(dim=dim, keepdim=True).values).to(torch.uint8).argmax(dim=dim).to(torch.int32)


def stats(x):
    """[n, 2]: {max(|x_n|, eps), |x_n| >= eps} (t64_stats)"""
    n = x.detach().norm(dim=1)
    return torch.stack([n.clamp_min(EPS), (n >= EPS).to(x.dtype)], dim=1)


def three(fn):
    """(float64, fp32 at 16 threads, fp32 at 1 thread)"""
    return fn(torch.float64), _with_threads(16, lambda: fn(torch.float32)), _with_threads(1, lambda: fn(torch.float32))


# ---- ProtoMF -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sim_inputs(R, D, P, lookup):
    table, rows, protos = protomf_inputs.argmin_safe(R, D, P, seed=R + D + P)
    G = torch.randn(R, P, generator=torch.Generator().manual_seed(R)) / R
    return dict(table=table, rows=rows if lookup else None, protos=protos, G=G)


def gathered(inp):
    return inp['table'] if inp['rows'] is None else inp['table'][inp['rows'].long()]


def sim_ref(inp, dtype):
    e, p = gathered(inp).to(dtype).clone().requires_grad_(True), inp['protos'].to(dtype).clone().requires_grad_(True)
    sim = protomf_ref.shifted_cosine_sim(e, p)
    pl, bl = protomf_ref.reg_losses(sim)
    ((sim * inp['G'].to(dtype)).sum() + W_PROTO * pl + W_BATCH * bl).backward()
    dis = 2 - sim.detach()
    return dict(sim=sim.detach(), cos_raw=(F.normalize(e) @ F.normalize(p).T).detach(), row_stat=stats(e), proto_stat=stats(p),
                row_best=lowest_arg(dis, 1), col_best_val=dis.min(dim=0).values, col_best_row=lowest_arg(dis, 0),
                proto_loss=pl.detach().reshape(1), batch_loss=bl.detach().reshape(1), dE=e.grad, dP=p.grad)


def sim_precondition(inp):
    e, p = gathered(inp).double(), inp['protos'].double()
    row_m, col_m = protomf_inputs.margins(e, p)
    if e.shape[1] == 1:
        assert protomf_inputs.exact_only(row_m) and protomf_inputs.exact_only(col_m), 'D = 1: margins are exactly 0 or 2'
    else:
        assert float(row_m.min()) >= protomf_inputs.MARGIN and float(col_m.min()) >= protomf_inputs.MARGIN, 'precondition: arg-min margins'


# ---- ProtoMFs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_inputs(R, D, P, fan, with_widx, lookup):
    """tests/test_hip_protomfs.py's inputs: weights exactly 0 (one in five) or |w| >= KINK; rows and widx name some rows twice"""
    gen = torch.Generator().manual_seed(R + D + P + fan)
    n_table = R + 3 if lookup else R
    table, protos = torch.randn(n_table, D, generator=gen), torch.randn(P, D, generator=gen)
    rows = _dups(torch.randperm(n_table, generator=gen)[:R]) if lookup else None
    if fan == 0:
        return dict(table=table, rows=rows, protos=protos, wt=None, widx=None, G=torch.randn(R, P, generator=gen) / R)
    n_w = R * fan + 2 if with_widx else R * fan
    wt = torch.randn(n_w, P, generator=gen)
    wt = torch.where(wt.abs() < KINK, torch.full_like(wt, KINK), wt)
    wt[torch.rand(wt.shape, generator=gen) < 0.2] = 0.
    widx = _dups(torch.randperm(n_w, generator=gen)[:R * fan]) if with_widx else None
    return dict(table=table, rows=rows, protos=protos, wt=wt, widx=widx, G=torch.randn(R, fan, generator=gen) / R)


def score_ref(inp, dtype):
    e, p = gathered(inp).to(dtype).clone().requires_grad_(True), inp['protos'].to(dtype).clone().requires_grad_(True)
    out = dict(cos_raw=(F.normalize(e) @ F.normalize(p).T).detach(), row_stat=stats(e), proto_stat=stats(p))
    if inp['wt'] is None:
        cos = protomfs_ref.cosine_sim(e, p)
        (cos * inp['G'].to(dtype)).sum().backward()
        out.update(cos=cos.detach())
    else:
        R, fan = inp['G'].shape
        w = (inp['wt'] if inp['widx'] is None else inp['wt'][inp['widx'].long()]).to(dtype).reshape(R, fan, -1).clone().requires_grad_(True)
        o = protomfs_ref.score(e, p, w)
        (o * inp['G'].to(dtype)).sum().backward()
        out.update(out=o.detach(), dWrows=w.grad.reshape(R * fan, -1))
    out.update(dE=e.grad, dP=p.grad)
    return out


def cos_precondition(e, others):
    """every |cos| <= 1 - KINK in float64, so no clamp decision can differ; D = 1: every cosine is exactly +-1 in every precision"""
    cos = F.normalize(e.double()) @ F.normalize(others.double()).T
    if e.shape[1] == 1:
        assert bool((cos.abs() == 1).all()), 'D = 1: cosines are exactly +-1'
    else:
        assert float(cos.abs().max()) <= 1 - KINK, 'precondition: cosines at the clamp'


def score_precondition(inp):
    cos_precondition(gathered(inp), inp['protos'])
    if inp['wt'] is not None:
        w = inp['wt'].double()
        assert bool(((w == 0) | (w.abs() >= KINK)).all()), 'precondition: weights at the ReLU kink'


# ---- ACF ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def anchor_inputs(R, D, K, lookup):
    gen = torch.Generator().manual_seed(R + D + K)
    n_table = R + 3 if lookup else R
    table, anchors = torch.randn(n_table, D, generator=gen), torch.randn(K, D, generator=gen)
    rows = _dups(torch.randperm(n_table, generator=gen)[:R]) if lookup else None
    return dict(table=table, rows=rows, anchors=anchors, G=torch.randn(R, D, generator=gen) / R)


def anchor_ref(inp, dtype, loss):
    e, a = gathered(inp).to(dtype).clone().requires_grad_(True), inp['anchors'].to(dtype).clone().requires_grad_(True)
    r, c, s = acf_ref.mix(e, a)
    obj = (r * inp['G'].to(dtype)).sum()
    out = dict(r=r.detach(), c=c.detach())
    if loss:
        exc, inc = acf_ref.losses(c, s)
        obj = obj + W_EXC * exc + W_INC * inc
        q = acf_ref.q_of(c.detach())
        out.update(lse=torch.logsumexp(s.detach(), dim=-1), q=q, dinc=torch.log(q) / c.detach().sum(), exc=exc.detach().reshape(1),
                   inc=inc.detach().reshape(1))
    obj.backward()
    out.update(dE=e.grad, dA=a.grad)
    return out


def anchor_precondition(inp):
    c = acf_ref.mix(gathered(inp).double(), inp['anchors'].double())[1]
    assert float(acf_ref.q_of(c).min()) > 0, 'precondition: every anchor takes some mass in float64 (an empty one gives inc = NaN)'


# ---- ECF ---------------------------------------------------------------------------------------------------------------------------------
CLUSTER_SEED_SHIFT = {(65, 64, 192, 96): 1}        # the plain seed leaves 2 of 65 rows out (3.08 %); chosen on the float64 reference alone


@functools.lru_cache(maxsize=None)
def cluster_inputs(R, D, C, top):
    """cosine form; ``keep``: the rows whose float64 gap at the mask boundary is >= NEAR_TIE. The upstream gradients of the others are
    zero, so they reach neither dW nor dCl, and their rows of t, x and the mask are not compared."""
    gen = torch.Generator().manual_seed(R + D + C + top + CLUSTER_SEED_SHIFT.get((R, D, C, top), 0))
    W, Cl = torch.randn(R, D, generator=gen), torch.randn(C, D, generator=gen)
    G, Gt = torch.randn(R, C, generator=gen) / R, torch.randn(R, C, generator=gen) / R
    keep = ecf_ref.gap(ecf_ref.cosine_sim(W.double(), Cl.double()), top) >= NEAR_TIE
    return dict(W=W, Cl=Cl, G=G * keep[:, None], Gt=Gt * keep[:, None], keep=keep, top=top)


@functools.lru_cache(maxsize=None)
def logit_inputs(R, C, top):
    gen = torch.Generator().manual_seed(R + C + top)
    return dict(t=torch.randn(R, C, generator=gen) * 2.0, G=torch.randn(R, C, generator=gen) / R, top=top)


def mask_bytes(m):
    """[R, ceil(C / 4)] uint8: bits 0 .. 3 of byte q = m of clusters 4 q .. 4 q + 3 (the clamp bits 4 .. 7 are zero under cos_precondition)"""
    R, C = m.shape
    C4 = (C + 3) // 4
    bits = torch.zeros(R, 4 * C4, dtype=torch.int32)
    bits[:, :C] = (m != 0).to(torch.int32)
    return (bits.reshape(R, C4, 4) * torch.tensor([1, 2, 4, 8], dtype=torch.int32)).sum(dim=-1).to(torch.uint8)


def _row_state(t, norms):
    z = t.detach() / TEMP
    m = z.max(dim=1).values
    return torch.cat([torch.stack([m, torch.exp(z - m[:, None]).sum(dim=1)], dim=1), norms], dim=1)


def cluster_ref(inp, dtype):
    w, c = inp['W'].to(dtype).clone().requires_grad_(True), inp['Cl'].to(dtype).clone().requires_grad_(True)
    t = ecf_ref.cosine_sim(w, c)
    m = ecf_ref.top_mask(t, inp['top'])
    p = torch.softmax(t / TEMP, dim=-1)
    x = torch.sigmoid(t) * (p + (m - p).detach())
    ((x * inp['G'].to(dtype)).sum() + (t * inp['Gt'].to(dtype)).sum()).backward()
    return dict(t=t.detach(), x=x.detach(), row_state=_row_state(t, stats(w)), mask=mask_bytes(m), dW=w.grad, dCl=c.grad)


def logit_ref(inp, dtype):
    t = inp['t'].to(dtype).clone().requires_grad_(True)
    x = ecf_ref.affiliation(t, inp['top'], TEMP)
    (x * inp['G'].to(dtype)).sum().backward()
    return dict(x=x.detach(), row_state=_row_state(t, torch.zeros(len(t), 2, dtype=dtype)), mask=mask_bytes(ecf_ref.top_mask(t.detach(), inp['top'])),
                dt=t.grad)


def cluster_precondition(inp):
    share = 1.0 - float(inp['keep'].double().mean())
    assert share <= NEAR_TIE_CAP, f'near-tie rows left out: {share:.4f}'
    cos_precondition(inp['W'], inp['Cl'])
    return share


def logit_precondition(inp):
    assert float(ecf_ref.gap(inp['t'], inp['top']).min()) > 0, 'precondition: no tie at the mask boundary (the inputs are the same fp32 values)'


# ---- derived forward-error bounds ----------------------------------------------------------------------------------------------------------
# Three tensors have legitimate max-norm ratios above KAPPA on the MI355X: a scalar (exc) or a tensor of a few hundred elements (lse and t
# at N = 2) whose fp32 CPU error happens to be a fraction of an ulp, while the kernel's is an ordinary 1 - 2 ulp (measured: exc 8.61 at
# (129, 65, 129), lse 3.99 and t 4.35 at (129, 512, 2)). The CPU error is then no yardstick, and their bound is a first-order forward-error
# bound instead, u = 2^-24, the same expression on absolute values in float64, the constants counted from the kernels' operation chains
# (the convention of tests/test_hip_rowops.py and tests/test_hip_tail.py). They are worst-case bounds: a D-term FMA chain is charged D u,
# so they are loose by the usual factor against the observed errors, and still orders of magnitude below what a dropped chunk, row or
# column does to the value.
U32 = 2.0 ** -24
EXP_U = 4                                          # expf / logf: 2 ulp = 4 u relative (hip_testutil.EXP_ULP)


def cluster_t_bound(inp):
    """t = clamp(w . c / (|w| |c|)). The dot product is a chain of D FMAs: D u sum_d |w_d c_d|. Each squared norm is a sum of D terms
    (<= D u relative, whatever the tree), the square root halves that and adds u, the product of the two norms and the division add u each:
    (D + 4) u relative on the quotient. With A = sum_d |w_d c_d| / (|w| |c|) >= |t|:   |err| <= (2 D + 4) u A.   The clamp is 1-Lipschitz."""
    w, c = inp['W'].double().abs(), inp['Cl'].double().abs()
    return (2 * w.shape[1] + 4) * U32 * (F.normalize(w) @ F.normalize(c).T)


def anchor_loss_bounds(inp):
    """-> {'lse': [R], 'exc': [1]}. s = e A^T by a chain of D FMAs: E_s[j, k] = D u sum_d |e_d a_d|. With m = max_k s, x_k = s_k - m,
    c = softmax(s), X = sum_k c_k |x_k|:
      lse = m + log(sum_k exp(x_k)) is a c-weighted mean in s (max_k E_s), x_k rounds once and expf has EXP_U (relative X u + EXP_U u on
      the sum), the sum of K terms K u, logf EXP_U u |lse - m|, the last addition u |lse|:
          |err lse| <= max_k E_s + u (X + K + EXP_U + EXP_U |lse - m| + |lse|)                                        =: B_lse
      H = - sum_k c_k (s_k - lse), dH / ds_k = - c_k (s_k - lse + H): sum_k c_k |s_k - lse + H| E_s[k] for the logits; each c_k carries
      (max_k |x_k| + EXP_U + K + 1) u relative (argument, expf, the sum, the division), s_k - lse rounds once, the FMA chain and the
      row-group tree over K terms K u, all on L = sum_k c_k |s_k - lse|; the evaluation error of lse enters once (sum_k c_k = 1):
          |err H| <= sum_k c_k |s_k - lse + H| E_s[k] + u (max_k |x_k| + 2 K + EXP_U + 2) L + (B_lse - max_k E_s)
      exc = mean_j H_j is summed in double and rounded once: mean_j |err H_j| + u |exc|."""
    e, a = gathered(inp).double(), inp['anchors'].double()
    D, K = e.shape[1], a.shape[0]
    s = e @ a.T
    E_s = D * U32 * (e.abs() @ a.abs().T)
    m = s.max(dim=1, keepdim=True).values
    c = torch.softmax(s, dim=1)
    lse = torch.logsumexp(s, dim=1, keepdim=True)
    X = (c * (s - m).abs()).sum(dim=1, keepdim=True)
    ev_lse = U32 * (X + K + EXP_U + EXP_U * (lse - m).abs() + lse.abs())
    H = -(c * (s - lse)).sum(dim=1, keepdim=True)
    L = (c * (s - lse).abs()).sum(dim=1, keepdim=True)
    err_H = (c * (s - lse + H).abs() * E_s).sum(dim=1, keepdim=True) + U32 * ((s - m).abs().max(dim=1, keepdim=True).values + 2 * K + EXP_U + 2) * L + ev_lse
    return dict(lse=(E_s.max(dim=1, keepdim=True).values + ev_lse).reshape(-1), exc=(err_H.mean() + U32 * H.mean().abs()).reshape(1))
