"""tests/bn_ref64.py without a device: the float64 reference against F.batch_norm(training=True) in float64 with autograd,
what torch's fp32 arithmetic costs on the same inputs (the ORACLE_* record of the module's docstring), the mask band of
every ReLU case of the GPU file, the strip rule's boundaries, and the refusals that need no kernel."""
import os
import socket

import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref64 as B
from tests import route_util as R


def _torch_bn(case, relu, dtype, eps=B.EPS, momentum=0.1):
    """F.batch_norm(training=True) (+ res, + ReLU) with autograd in `dtype`: y, new running stats, dz, dgamma, dbeta, dres"""
    z = case['z'].to(dtype).requires_grad_(True)
    gm = case['gamma'].to(dtype).requires_grad_(True)
    bt = case['beta'].to(dtype).requires_grad_(True)
    res = case['res'].to(dtype).requires_grad_(True) if case['res'] is not None else None
    rm, rv = case['rm'].to(dtype).clone(), case['rv'].to(dtype).clone()
    pre = F.batch_norm(z, rm, rv, gm, bt, True, momentum, eps)
    if res is not None:
        pre = pre + res
    y = pre.relu() if relu else pre
    y.backward(case['dout'].to(dtype))
    return dict(y=y.detach(), rm=rm, rv=rv, dz=z.grad, dgamma=gm.grad, dbeta=bt.grad,
                dres=res.grad if res is not None else None)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('residual', [False, True])
def test_reference_equals_torch_float64(relu, residual):
    case = B.make_case(273, 32, torch.float32, 3, residual=residual, constant=(4,))
    f = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, relu, case['res'], case['rm'], case['rv'], 0.1)
    b = B.bn_backward64(case['dout'], f, f.pre > 0 if relu else torch.ones_like(f.pre, dtype=torch.bool))
    t = _torch_bn(case, relu, torch.float64, eps=B.f32(B.EPS), momentum=B.f32(0.1))
    for name, mine, ref in (('y', f.y, t['y']), ('running_mean', f.new_rm, t['rm']), ('running_var', f.new_rv, t['rv']),
                            ('dz', b.dz, t['dz']), ('dgamma', b.dgamma, t['dgamma']), ('dbeta', b.dbeta, t['dbeta'])):
        err = (mine - ref).abs().max().item()
        assert err <= 1e-11 * max(1.0, ref.abs().max().item()), (name, err)
    if residual:
        assert torch.equal(b.dres, t['dres'])
    # the constant channel: var == 0 exactly, rstd finite through eps, kappa finite
    assert f.var[4].item() == 0.0 and f.rstd[4].item() == pytest.approx(B.f32(B.EPS) ** -0.5) and f.kappa[4].item() == 0.0


def test_momentum_none_is_the_cumulative_average():
    """m = 1 / num_batches_tracked, computed on the host: three calls give the plain average of the batch statistics"""
    bn = torch.nn.BatchNorm2d(8, momentum=None).double()
    rm, rv = torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    for k in range(1, 4):
        case = B.make_case(49, 8, torch.float32, 50 + k)
        bn(case['z'].double().t().reshape(1, 8, 7, 7))
        f = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, False, None, rm, rv, 1.0 / k)
        rm, rv = f.new_rm, f.new_rv
        assert int(bn.num_batches_tracked) == k
        # (m goes through a float on its way to the kernel: 1 / 3 differs from the double by 1e-8 of itself)
        assert (rm - bn.running_mean).abs().max().item() <= 1e-7 and (rv - bn.running_var).abs().max().item() <= 1e-7


def test_what_fp32_costs_stays_under_the_recorded_ceilings():
    """the ORACLE_* record: torch's fp32 F.batch_norm with autograd against the float64 reference; prints the ratios the
    docstring of bn_ref64 quotes and holds them under about twice those figures"""
    for i, mean in enumerate((0.3, 10.0, 100.0)):
        case = B.make_case(273, 32, torch.float32, 41, mean=mean)
        f = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, True, None, case['rm'], case['rv'], 0.1)
        t = _torch_bn(case, True, torch.float32)
        b = B.bn_backward64(case['dout'], f, t['y'] > 0)
        n = f.n
        rv1 = torch.zeros(32)           # momentum 1: the running variance IS the unbiased batch variance
        F.batch_norm(case['z'], torch.zeros(32), rv1, None, None, True, 1.0, B.EPS)
        var32 = rv1.double() * (n - 1.0) / n
        y_rel = ((t['y'].double() - f.y).abs().max() / max(1.0, f.y.abs().max().item())).item()
        y_cond = ((t['y'].double() - f.y).abs() / B.y_extra(f)).max().item()
        var_u = ((var32 - f.var).abs() / (B.U * f.var)).max().item()
        var_b = ((var32 - f.var).abs() / ((B.K_VAR + 1) * B.U * f.m2)).max().item()
        dz = ((t['dz'].double() - b.dz).abs() / B.dz_extra(f, b)).max().item()
        dgamma = ((t['dgamma'].double() - b.dgamma).abs() / B.dgamma_extra(f, b)).max().item()
        dbeta = ((t['dbeta'].double() - b.dbeta).abs() / (B.U * b.S_beta)).max().item()
        print(f'mean {mean}: kappa {f.kappa.min().item():.2f}-{f.kappa.max().item():.2f}  y_rel {y_rel:.2e}  y/extra {y_cond:.3f}  '
              f'var/u {var_u:.3f}  var/bound {var_b:.4f}  dz/extra {dz:.3f}  dgamma/extra {dgamma:.3f}  dbeta/(u S) {dbeta:.3f}')
        assert y_rel <= B.ORACLE_Y_REL[i]
        assert y_cond <= B.ORACLE_Y_OVER_EXTRA
        assert var_u <= B.ORACLE_VAR[i]
        assert var_b <= B.ORACLE_VAR_OVER_BOUND
        assert dz <= B.ORACLE_DZ_OVER_EXTRA
        assert dgamma <= B.ORACLE_DGAMMA_OVER_EXTRA
        assert dbeta <= B.ORACLE_DBETA


def test_pivot_keeps_kappa_small_where_mean_squared_over_var_is_large():
    """the conditioning the bounds scale with is the pivot's, not mean^2 / var: 1e4 there, below 20 here"""
    case = B.make_case(273, 64, torch.float32, 31, mean=100.0)
    f = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, False)
    assert (f.mean ** 2 / f.var).min().item() > 5e3
    assert f.kappa.max().item() < 20.0


@pytest.mark.parametrize('name', [k for k, s in B.cases().items() if s['relu'] and s['rows'] <= 20000])
def test_mask_band_of_every_relu_case(name):
    spec = B.cases()[name]
    case = B.case_inputs(spec)
    f = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, True, case['res'])
    share = B.mask_band_share(f, spec['dtype'])
    assert share <= B.MASK_BAND_CAP, (name, share)


def test_strip_rule_boundaries():
    f32, bf = torch.float32, torch.bfloat16
    assert B.plan(32, 4, f32)[4:] == (1, 32) and B.plan(33, 4, f32)[4:] == (2, 32)
    assert B.plan(16383, 8, bf)[4] == 512 and B.plan(16384, 8, bf)[4:] == (256, 64)
    assert B.plan(131073, 8, bf)[4:] == (511, 257)
    assert B.plan(1050, 2048, f32)[:4] == (4, 64, 4, 8) and B.plan(1050, 2048, bf)[:4] == (8, 64, 4, 4)
    # the shapes that are there for the fold into doubles reach a second chain; the one-vector widths never do
    assert B.chain(131073, 64, f32) == (16, 2) and B.chain(34817, 512, bf) == (16, 2)
    assert all(B.chain(r, B.MIN_C[bf], bf)[1] == 1 for r in B.ROW_COUNTS)


def test_mutations_differ_from_the_reference_by_more_than_the_bounds():
    """the two wrong references of the GPU file's mutation legs, on the CPU: the bounds can tell them from the right one"""
    case = B.make_case(49, 8, torch.float32, 7)
    f = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, False, None, case['rm'], case['rv'], 0.1)
    w = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, False, None, case['rm'], case['rv'], 0.1, biased_running=True)
    assert ((w.new_rv - f.new_rv).abs() / B.running_var_bound(f)).min().item() > 10
    mask = torch.ones_like(f.pre, dtype=torch.bool)
    b, wb = B.bn_backward64(case['dout'], f, mask), B.bn_backward64(case['dout'], f, mask, drop_dgamma_term=True)
    assert ((wb.dz - b.dz).abs() / R.bound(b.dz, torch.float32, B.dz_extra(f, b))).max().item() > 10


# ---- refusals that need no kernel ------------------------------------------------------------------------------------------
def test_out_of_scope_forms_raise_their_own_errors():
    import brcnn  # noqa: F401
    from brcnn.autograd import bn_train_act_autograd
    z = torch.randn(2, 3, 3, 8)
    with pytest.raises(NotImplementedError, match='track_running_stats'):
        bn_train_act_autograd(z, torch.nn.BatchNorm2d(8, track_running_stats=False))
    with pytest.raises(NotImplementedError, match='affine'):
        bn_train_act_autograd(z, torch.nn.BatchNorm2d(8, affine=False))
    bn = torch.nn.BatchNorm2d(8)
    with pytest.raises(NotImplementedError, match='HIP path'):      # a host tensor: no quiet torch fall-back
        bn_train_act_autograd(z, bn)
    assert int(bn.num_batches_tracked) == 0


def test_build_norm_layer_remembers_the_configured_type():
    import brcnn  # noqa: F401
    from brcnn.autograd import sync_bn_across_ranks
    from brcnn.blocks import build_norm_layer
    assert build_norm_layer(dict(type='SyncBN', requires_grad=True), 8)[1].brcnn_norm_type == 'SyncBN'
    bn = build_norm_layer(dict(type='BN'), 8)[1]
    assert bn.brcnn_norm_type == 'BN' and 'brcnn_norm_type' not in bn.state_dict()
    assert not sync_bn_across_ranks(build_norm_layer(dict(type='SyncBN'), 8)[1])        # no process group: one rank


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _syncbn_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import brcnn  # noqa: F401
        from brcnn.autograd import bn_train_act_autograd, sync_bn_across_ranks
        from brcnn.blocks import build_norm_layer
        sync, plain = build_norm_layer(dict(type='SyncBN'), 8)[1], build_norm_layer(dict(type='BN'), 8)[1]
        z = torch.randn(2, 3, 3, 8)
        try:
            bn_train_act_autograd(z, sync)
            raised = ''
        except NotImplementedError as e:
            raised = str(e)
        ret[rank] = (raised, sync_bn_across_ranks(sync), sync_bn_across_ranks(plain), int(sync.num_batches_tracked))
    finally:
        dist.destroy_process_group()


def test_syncbn_in_training_mode_under_two_ranks_raises():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_syncbn_worker, args=(world, port, ret), nprocs=world, join=True)
    for rank in range(world):
        raised, sync, plain, tracked = ret[rank]
        assert 'SyncBN' in raised and 'more than one rank' in raised
        assert sync and not plain and tracked == 0
