"""Host check of the reference helper the training-step GPU tests lean on (tests/train_ref.py: OracleGraph): fed the cotangents of
the Trainer's own loss it must give the Trainer's parameter gradients; where no path leads from the chosen outputs to a parameter
it must say so."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_ref import NAMES, OracleGraph, build_train_case, grad_err, stack_trainer_cotangents  # noqa: E402


@pytest.fixture(scope='module')
def case(specs):
    tc = build_train_case(specs)
    return tc, OracleGraph(tc['sd_r'], tc['fm'], tc['label'][:4], None, 4, dtype=torch.float32)


def test_trainer_cotangents_give_the_trainer_gradients(case):
    """sum_i <out_i, dLoss/dout_i> differentiated through the graph IS loss.backward(): the chain rule, in the arithmetic of
    build_train_case (fp32), to the bound test_train_backward_matches_oracle_and_golden puts on its own helper."""
    tc, graph = case
    for nm, o, a, b in zip(NAMES, graph.outs, tc['out_non'], tc['out_ocl']):
        assert torch.equal(o, torch.cat([a, b]).detach().reshape(o.shape)), nm      # the same forward, bit for bit
    got = graph.grads(stack_trainer_cotangents(tc))
    worst = max((grad_err(got[k], tc['param_grads'][k]), k) for k in tc['keys'])
    print('worst difference to build_train_case: %.2e (%s)' % worst)
    for k in tc['keys']:
        assert got[k] is not None, k                  # the Trainer's loss reaches all 76 parameters
        assert grad_err(got[k], tc['param_grads'][k]) < 1e-6, k


def test_parameters_without_a_path_come_back_as_none(case):
    """One output at a time: the parameters behind it are reported, the others are None, not zeros.  f_new does not see the
    classifier; M_space sees Conv4Space alone; M_channel sees Conv4Channel alone; all seven together see everything."""
    tc, graph = case
    g = torch.Generator().manual_seed(5)

    def reached(name):
        cots = [torch.randn(o.shape, generator=g) if nm == name or name == 'all' else None for nm, o in zip(NAMES, graph.outs)]
        return {k for k, v in graph.grads(cots).items() if v is not None}

    keys = set(tc['keys'])
    assert keys - reached('f_new') == {'classifier.weight'}
    assert reached('M_space') == {k for k in keys if k.startswith('Conv4Space.')} and len(keys - reached('M_space')) == 40
    assert reached('M_channel') == {k for k in keys if k.startswith('Conv4Channel.')} and len(keys - reached('M_channel')) == 61
    assert reached('feat_space') == reached('M_space')
    assert len(keys - reached('feat_channel')) == 49
    assert reached('pred_loss') == keys and reached('pred_label') == keys and reached('all') == keys
