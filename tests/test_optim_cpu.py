"""CPU: the optimizer tail's host side -- the argument checks of ds2_clip_adam and
ds2_clip_sgd_nesterov_wd (they return before any HIP call), FusedAdam's and FusedSGD's
torch-format state dicts on a CPU FlatParams, and build_optimizer (ref train.py:139-152).
The updates themselves run on the GPU: tests/test_gpu_optim.py.
"""
import copy
import ctypes
import os
import types

import pytest
import torch

from ds2amd import _lib
from ds2amd import model as dsm
from ds2amd.optim import FlatParams, FusedAdam, FusedSGD, build_optimizer

INVALID = 1     # DS2_INVALID_VALUE


# ------------------------------------------------------------------ argument checks
def _adam_args(step_ptr):
    # params, grads, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay,
    # max_norm, norm, step, skip_flag, stream
    return [None, None, None, None, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None, step_ptr, None,
            None]


@pytest.mark.parametrize("index,bad", [
    (4, -1),                                   # numel < 0
    (0, 4), (1, 8), (2, 4), (3, 12),           # a buffer not 16-byte aligned
    (12, None),                                # step == NULL
    (5, -1e-3), (8, -1e-8), (9, -1e-4),        # lr, eps, weight_decay < 0
    (6, -0.1), (6, 1.0), (7, 1.0), (7, 1.5), (7, -0.5),   # a beta outside [0, 1)
    (5, float('nan')), (6, float('nan')),
])
def test_clip_adam_rejects_bad_arguments(index, bad):
    lib = _lib.load()
    step = ctypes.c_int(0)
    args = _adam_args(ctypes.addressof(step))
    args[index] = bad
    assert lib.ds2_clip_adam(*args) == INVALID, (index, bad)
    assert step.value == 0


def test_clip_adam_numel_zero_is_ok_without_launch():
    lib = _lib.load()
    step = ctypes.c_int(5)
    args = _adam_args(ctypes.addressof(step))
    args[4] = 0
    assert lib.ds2_clip_adam(*args) == 0
    assert step.value == 5


@pytest.mark.parametrize("index,bad", [
    (3, -1), (0, 4), (1, 8), (2, 4), (4, -0.1), (6, -1e-4), (6, float('nan')),
])
def test_clip_sgd_nesterov_wd_rejects_bad_arguments(index, bad):
    lib = _lib.load()
    # params, grads, momentum_buf, numel, lr, momentum, weight_decay, max_norm, norm, skip, stream
    args = [None, None, None, 16, 0.1, 0.9, 1e-4, 1.0, None, None, None]
    args[index] = bad
    assert lib.ds2_clip_sgd_nesterov_wd(*args) == INVALID, (index, bad)


def test_clip_sgd_nesterov_wd_numel_zero_is_ok_without_launch():
    lib = _lib.load()
    assert lib.ds2_clip_sgd_nesterov_wd(None, None, None, 0, 0.1, 0.9, 1e-4, 1.0, None, None,
                                        None) == 0


# ------------------------------------------------------------------ state dicts
@pytest.fixture(scope="module")
def resume_pkg(golden_dir):
    return torch.load(os.path.join(golden_dir, 'tiny_ref_resume.pth'), map_location='cpu',
                      weights_only=True)


def _torch_adam_after_two_steps(pkg, **kw):
    """A torch copy of the package's model, two seeded torch.optim.Adam steps."""
    m = dsm.DeepSpeech.load_model_package(pkg)
    params = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    opt = torch.optim.Adam(params, **kw)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return params, opt


def _fused_adam(pkg, **kw):
    m = dsm.DeepSpeech.load_model_package(pkg)
    flat = FlatParams(list(m.parameters()), 'cpu')
    return m, flat, FusedAdam(flat, **kw)


def test_fused_adam_state_dict_is_torch_adam_format(resume_pkg):
    """FusedAdam (flat buffers, reverse layer order inside) loads torch.optim.Adam's dict and
    writes back exactly that format in model.parameters() order; torch's own Adam accepts
    what it writes; the set_lr round trip (train.py:322-326) changes lr alone."""
    params, topt = _torch_adam_after_two_steps(resume_pkg, lr=2e-3, betas=(0.8, 0.99), eps=1e-7,
                                               weight_decay=1e-4)
    ref = topt.state_dict()
    m, flat, opt = _fused_adam(resume_pkg, lr=1.0)
    assert opt.state_dict()['state'] == {}           # no step counted yet
    opt.load_state_dict(ref)
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay) == (2e-3, (0.8, 0.99), 1e-7, 1e-4)
    assert int(opt.step_count) == 2
    ours = opt.state_dict()
    assert sorted(ours) == ['param_groups', 'state']
    assert len(ours['param_groups']) == 1
    assert sorted(ours['param_groups'][0]) == sorted(ref['param_groups'][0])
    for k, v in ref['param_groups'][0].items():
        assert ours['param_groups'][0][k] == v, k
    assert sorted(ours['state']) == sorted(ref['state']) == list(range(len(params)))
    for i, st in ref['state'].items():
        mine = ours['state'][i]
        assert sorted(mine) == sorted(st)
        assert torch.is_tensor(mine['step']) and mine['step'].dtype == torch.float32
        assert mine['step'].shape == () and float(mine['step']) == float(st['step']) == 2.0
        assert torch.equal(mine['exp_avg'], st['exp_avg']), i
        assert torch.equal(mine['exp_avg_sq'], st['exp_avg_sq']), i
    # inside, the flat layout is reversed: the LAST parameter's moments come first
    last = list(m.parameters())[-1]
    assert flat.offset_of[id(last)] == 0
    assert torch.equal(opt.exp_avg[:last.numel()].view_as(last),
                       ref['state'][len(params) - 1]['exp_avg'])
    # torch's own Adam loads what we write
    fresh = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=0.5)
    fresh.load_state_dict(ours)
    assert fresh.param_groups[0]['lr'] == 2e-3
    assert torch.equal(fresh.state[fresh.param_groups[0]['params'][3]]['exp_avg_sq'],
                       ref['state'][3]['exp_avg_sq'])
    # set_lr: state_dict -> edit lr -> load_state_dict
    sd = opt.state_dict()
    sd['param_groups'][0]['lr'] = 1e-5
    opt.load_state_dict(sd)
    again = opt.state_dict()
    assert opt.lr == 1e-5 and again['param_groups'][0]['lr'] == 1e-5
    for k, v in ours['param_groups'][0].items():
        if k != 'lr':
            assert again['param_groups'][0][k] == v, k
    for i, st in ours['state'].items():
        for k in st:
            assert torch.equal(again['state'][i][k], st[k]), (i, k)


def _refusals(ref):
    def edit(fn):
        sd = copy.deepcopy(ref)
        fn(sd)
        return sd

    def group(key, value):
        return edit(lambda sd: sd['param_groups'][0].__setitem__(key, value))

    sgd = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1, momentum=0.9,
                          nesterov=True).state_dict()
    return {
        "another optimizer's dict (no betas)": sgd,
        "not a state_dict": {'lr': 1.0, 'betas': (0.9, 0.999)},
        "amsgrad": group('amsgrad', True),
        "maximize": group('maximize', True),
        "decoupled_weight_decay": group('decoupled_weight_decay', True),
        "parameter count": edit(lambda sd: sd['param_groups'][0]['params'].pop()),
        "shape": edit(lambda sd: sd['state'][2].__setitem__(
            'exp_avg', sd['state'][2]['exp_avg'].reshape(-1)[:-1].clone())),
        "shape (second moment)": edit(lambda sd: sd['state'][0].__setitem__(
            'exp_avg_sq', torch.zeros(3))),
        "unknown state key": edit(lambda sd: sd['state'][1].__setitem__(
            'max_exp_avg_sq', torch.zeros_like(sd['state'][1]['exp_avg']))),
        "state for some parameters only": edit(lambda sd: sd['state'].pop(4)),
        "differing step": edit(lambda sd: sd['state'][5].__setitem__('step', torch.tensor(3.0))),
    }


def test_fused_adam_load_state_dict_refusals(resume_pkg):
    """Every dict FusedAdam cannot represent raises ValueError and leaves it as it was."""
    _, topt = _torch_adam_after_two_steps(resume_pkg, lr=2e-3)
    ref = topt.state_dict()
    _, _, opt = _fused_adam(resume_pkg, lr=1.0)
    opt.load_state_dict(ref)
    before = opt.state_dict()
    cases = _refusals(ref)
    assert len(cases) == 11
    for name, bad in cases.items():
        with pytest.raises(ValueError):
            opt.load_state_dict(bad)
        after = opt.state_dict()
        assert after['param_groups'] == before['param_groups'], name
        for i, st in before['state'].items():
            for k in st:
                assert torch.equal(after['state'][i][k], st[k]), (name, i, k)


def test_fused_adam_constructor_checks(resume_pkg):
    m = dsm.DeepSpeech.load_model_package(resume_pkg)
    flat = FlatParams(list(m.parameters()), 'cpu')
    for kw in (dict(lr=-1.0), dict(lr=1e-3, eps=-1.0), dict(lr=1e-3, betas=(1.0, 0.999)),
               dict(lr=1e-3, betas=(0.9, -0.1)), dict(lr=1e-3, weight_decay=-1e-4)):
        with pytest.raises(ValueError):
            FusedAdam(flat, **kw)


def test_fused_sgd_weight_decay_state_dict(resume_pkg):
    """A torch.optim.SGD(nesterov=True, weight_decay=1e-4) dict loads, the decay is adopted
    and reported back, torch's SGD loads the result; nesterov=False is still refused."""
    m = dsm.DeepSpeech.load_model_package(resume_pkg)
    params = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    topt = torch.optim.SGD(params, lr=0.05, momentum=0.8, nesterov=True, weight_decay=1e-4)
    g = torch.Generator().manual_seed(6)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    topt.step()
    ref = topt.state_dict()
    flat = FlatParams(list(m.parameters()), 'cpu')
    opt = FusedSGD(flat, lr=1.0, momentum=0.5)
    assert opt.weight_decay == 0 and opt.state_dict()['param_groups'][0]['weight_decay'] == 0
    opt.load_state_dict(ref)
    assert (opt.lr, opt.momentum, opt.weight_decay) == (0.05, 0.8, 1e-4)
    ours = opt.state_dict()
    for k, v in ref['param_groups'][0].items():
        assert ours['param_groups'][0][k] == v, k
    for i, st in ref['state'].items():
        assert torch.equal(ours['state'][i]['momentum_buffer'], st['momentum_buffer']), i
    sgd = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in params], lr=0.1,
                          momentum=0.9, nesterov=True)
    sgd.load_state_dict(ours)
    assert sgd.param_groups[0]['weight_decay'] == 1e-4
    assert FusedSGD(flat, lr=0.1, weight_decay=1e-4).state_dict()['param_groups'][0][
        'weight_decay'] == 1e-4
    bad = opt.state_dict()
    bad['param_groups'][0]['nesterov'] = False
    with pytest.raises(ValueError):
        opt.load_state_dict(bad)
    for key, value in (('dampening', 0.1), ('maximize', True), ('weight_decay', -1e-4)):
        bad = opt.state_dict()
        bad['param_groups'][0][key] = value
        with pytest.raises(ValueError):
            opt.load_state_dict(bad)
    assert opt.weight_decay == 1e-4


# ------------------------------------------------------------------ build_optimizer
def test_build_optimizer_mirrors_the_reference(resume_pkg):
    m = dsm.DeepSpeech.load_model_package(resume_pkg)
    flat = FlatParams(list(m.parameters()), 'cpu')
    args = types.SimpleNamespace(optimizer='sgd', lr=3e-4, momentum=0.85, weight_decay=1e-5)
    sgd = build_optimizer(args, flat, max_norm=400.0)
    assert type(sgd) is FusedSGD
    assert (sgd.lr, sgd.momentum, sgd.weight_decay, sgd.max_norm) == (3e-4, 0.85, 1e-5, 400.0)
    assert sgd.state_dict()['param_groups'][0]['nesterov'] is True
    args.optimizer = 'adam'
    adam = build_optimizer(args, flat, max_norm=400.0)
    assert type(adam) is FusedAdam
    # train.py:152 passes lr alone: torch's defaults for the rest, no decay
    assert (adam.lr, adam.betas, adam.eps, adam.weight_decay, adam.max_norm) == \
        (3e-4, (0.9, 0.999), 1e-8, 0.0, 400.0)
    args.optimizer = 'rmsprop'
    with pytest.raises(ValueError):
        build_optimizer(args, flat, max_norm=400.0)
