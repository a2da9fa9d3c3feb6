"""The training backward (include/ffrnet_train.h) driven every way a caller can drive it, not only the Trainer's way: each of the
seven output cotangents alone and all together, fold_channel = 0, loss weights other than ones, labels that hit and triplets
that do not, and the order of calls on the two context slots.  Everything at G = 2 groups of N = 3 images (147 rows per BatchNorm
batch: the smallest shape at which every kernel of the step still has ragged slices), against the float64 oracle
(oracle/ffr_oracle_train.py under torch autograd, tests/train_ref.py: OracleGraph) on the GPU's side of every PReLU kink."""
import os
import sys

import numpy as np
import pytest
import torch

import ffrnet_amd
from ffrnet_amd import synth
from ffrnet_amd.train import FlatBuffer

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_ref import NAMES, OracleGraph, check_kinks, gpu_kink_masks, grad_err, rel  # noqa: E402

G, N = 2, 3
TOL = 1e-4                           # per tensor, both arithmetics: the bound of test_train_backward_matches_oracle_and_golden
FWD_TOL = {0: 1e-5, 1: 1e-4}         # its forward tolerances for check_kinks: direct, Winograd


class World(object):
    """The fixed inputs, one engine, and the oracle's graphs: the natural one (its own side of every kink) and one per sign
    pattern a GPU forward produced, each built once and differentiated once per set of cotangents."""

    def __init__(self, specs):
        self.sd_r = synth.synth_state_dict(specs['recnet'], seed=0)
        g = torch.Generator().manual_seed(40 + N)
        self.fm = torch.randn(G * N, 512, 7, 7, generator=g) * 0.6
        self.label = torch.randint(0, 10575, (N,), generator=g).repeat(G)
        self.eng = ffrnet_amd.Engine(0)
        self.oracle = dict(device=self.eng.device, dtype=torch.float64)
        self.natural = OracleGraph(self.sd_r, self.fm, self.label, None, N, G, **self.oracle)
        self._graphs = []

    def graph_for(self, masks):
        for m, graph in self._graphs:
            if all(torch.equal(m[k], masks[k]) for k in m):
                return graph
        self._graphs.append((masks, OracleGraph(self.sd_r, self.fm, self.label, masks, N, G, **self.oracle)))
        return self._graphs[-1][1]

    def forward(self, wino=1, fold=1, want=()):
        """train_init, the options, the forward into slot 0 -> (outputs, the oracle on the GPU's side of every kink)."""
        eng = self.eng
        eng.train_init(self.sd_r)
        eng.train_option('winograd', wino)
        eng.train_option('fold_channel', fold)
        outs = eng.train_forward(self.fm.cuda(), self.label.cuda(), groups=G, want=want)
        masks = gpu_kink_masks(eng, G, N)
        flipped = check_kinks({k: m.to(self.oracle['device']) for k, m in masks.items()}, self.natural.pre, FWD_TOL[wino])
        return outs, self.graph_for(masks), flipped

    def cotangents(self, graph, names):
        """Seeded randn for the outputs in `names`, None elsewhere, divided by the largest entry of any parameter gradient the
        ORACLE gives for them (the backward is linear in the cotangent): the case's largest reference entry is 1, so the floor
        of grad_err (1e-3) is a thousandth of it.  -> (cotangents on the device, {key: reference gradient or None})"""
        cots = [torch.randn(o.shape, generator=torch.Generator().manual_seed(900 + i)) if nm in names else None
                for i, (nm, o) in enumerate(zip(NAMES, graph.outs))]
        ref = graph.grads(cots)
        top = max(v.abs().max().item() for v in ref.values() if v is not None)
        return [c.div(top).cuda() if c is not None else None for c in cots], {k: v / top if v is not None else None for k, v in ref.items()}

    def compare(self, ref, tag):
        """Every parameter gradient of the engine against `ref`; None = no path: exactly zero.  -> worst error"""
        worst, smallest, no_path = ('', 0.0), 1.0, 0
        for k, r in ref.items():
            got = self.eng.train_get(k, 'grad')
            if r is None:
                no_path += 1
                assert torch.equal(got, torch.zeros_like(got)), (tag, k, 'no path from these outputs, but', got.abs().max().item())
                continue
            e = grad_err(got, r.cpu())
            worst = max(worst, (k, e), key=lambda t: t[1])
            smallest = min(smallest, r.abs().max().item())
            assert e < TOL, (tag, k, e)
        print('%s: worst per-tensor error %.2e (%s); %d parameters without a path, all exactly zero; smallest per-tensor '
              'maximum %.1e of the largest' % (tag, worst[1], worst[0], no_path, smallest))
        return worst[1]

    def flat_grads(self, eng=None):
        info = (eng or self.eng).train_info()
        return torch.as_tensor(FlatBuffer(info['grads'], info['n_flat']), device=(eng or self.eng).device)


@pytest.fixture(scope='module')
def world(specs):
    w = World(specs)
    yield w
    w.eng.train_option('winograd', 1)
    w.eng.train_option('fold_channel', 1)


def fold_names(plan):
    return [p['name'] for p in plan if 'fold' in p['name']]


NO_PATH = {'f_new': 1, 'pred_loss': 0, 'pred_label': 0, 'M_space': 40, 'M_channel': 61, 'feat_space': 40, 'feat_channel': 49, 'all': 0}
CASES = [(nm, 1) for nm in NAMES] + [('all', 1), ('all', 0)]


# ---- 2. one cotangent at a time, then all seven ---------------------------------------------------------------------
@pytest.mark.parametrize('which,wino', CASES, ids=['%s-w%d' % c for c in CASES])
def test_backward_of_each_output_cotangent(world, which, wino):
    """ffr_train_backward with exactly one cotangent (None elsewhere), and with all seven: every parameter gradient per tensor,
    parameters the chosen output cannot reach exactly zero (every backward kernel is linear in its incoming gradient).  Three of
    the seven (pred_label, M_space, M_channel) are zeros under the Trainer's loss, so launch_mspace_grad_in, the ext operand of
    launch_sigmoid_bwd_ext and the pred_label branch of k_cosface_dcos add something only here."""
    _, graph, flipped = world.forward(wino)
    names = NAMES if which == 'all' else [which]
    cots, ref = world.cotangents(graph, names)
    assert sum(v is None for v in ref.values()) == NO_PATH[which]
    world.eng.train_zero_grad()
    world.eng.train_backward(cots)
    torch.cuda.synchronize()
    world.compare(ref, '%s winograd=%d (%d kinks transplanted)' % (which, wino, flipped))
    if which == 'all':
        assert sorted(fold_names(world.eng.train_wgrad_plan())) == ['Conv4Channel.fold0', 'Conv4Channel.fold1']


def test_zero_cotangents_equal_none(world):
    """The nn.Module shell passes autograd's materialised zeros for pred_label, M_space and M_channel: beside the Trainer's
    four cotangents that gives the bits of passing None."""
    flats = []
    for zeros in (False, True):
        _, graph, _ = world.forward()
        cots, _ = world.cotangents(graph, ['f_new', 'pred_loss', 'feat_space', 'feat_channel'])
        if zeros:
            cots = [c if c is not None else torch.zeros(o.shape, device='cuda') for c, o in zip(cots, graph.outs)]
        world.eng.train_zero_grad()
        world.eng.train_backward(cots)
        torch.cuda.synchronize()
        flats.append(world.flat_grads().clone())
    assert flats[0].abs().max() > 0 and torch.equal(flats[0], flats[1])


def test_backward_adds_to_the_gradient_buffer(world):
    """The ADDS contract of ffr_train_backward: backward(A), a fresh forward, backward(B) with no zero_grad between them gives
    oracle(A) + oracle(B)."""
    _, graph, _ = world.forward()
    cots_a, ref_a = world.cotangents(graph, ['pred_label', 'M_space'])
    cots_b, ref_b = world.cotangents(graph, ['f_new', 'M_channel'])
    world.eng.train_zero_grad()
    world.eng.train_backward(cots_a)
    world.eng.train_forward(world.fm.cuda(), world.label.cuda(), groups=G, want=())       # the same inputs: the same kink pattern
    world.eng.train_backward(cots_b)
    torch.cuda.synchronize()
    both = {}
    for k in ref_a:
        parts = [r for r in (ref_a[k], ref_b[k]) if r is not None]
        both[k] = sum(parts) if parts else None
    assert any(ref_a[k] is not None and ref_b[k] is not None for k in both)
    world.compare(both, 'backward(A) then backward(B)')


# ---- 3. fold_channel = 0 --------------------------------------------------------------------------------------------
def test_unfolded_conv4channel(world):
    """fold_channel = 0: the 512-wide intermediates of Conv4Channel formed as the reference forms them (t2, t5) and the four
    lin_backward calls that take the place of the two folded pairs -- outputs, t2, all gradients, and the plan record."""
    outs, graph, flipped = world.forward(fold=0, want=NAMES)
    torch.cuda.synchronize()
    for nm, got, want in zip(NAMES, outs, world.natural.outs):
        assert rel(got, want) < 2e-4, (nm, rel(got, want))
    assert rel(world.eng.train_debug('t2', (G * N * 512, 512)).reshape(G * N, 512, 512), world.natural.t2) < 2e-4
    cots, ref = world.cotangents(graph, NAMES)
    world.eng.train_zero_grad()
    world.eng.train_backward(cots)
    torch.cuda.synchronize()
    world.compare(ref, 'all, fold_channel=0 (%d kinks transplanted)' % flipped)
    plan = {p['name']: p for p in world.eng.train_wgrad_plan()}
    for i in (2, 3, 5, 6):
        assert plan['Conv4Channel.%d' % i]['path'] == 'plain-taps1', plan
    assert not fold_names(plan.values())


def test_backward_follows_the_forward_not_the_option(world):
    """A folded forward, fold_channel = 0 set before its backward: the backward is the folded one (what the forward recorded
    decides, not the option's value when the backward runs)."""
    _, graph, flipped = world.forward(fold=1)
    cots, ref = world.cotangents(graph, NAMES)
    world.eng.train_option('fold_channel', 0)
    try:
        world.eng.train_zero_grad()
        world.eng.train_backward(cots)
        torch.cuda.synchronize()
    finally:
        world.eng.train_option('fold_channel', 1)
    world.compare(ref, 'all, folded forward, fold_channel=0 at the backward')
    plan = [p['name'] for p in world.eng.train_wgrad_plan()]
    assert sorted(fold_names(world.eng.train_wgrad_plan())) == ['Conv4Channel.fold0', 'Conv4Channel.fold1']
    assert not any(nm in plan for nm in ('Conv4Channel.2', 'Conv4Channel.3', 'Conv4Channel.5', 'Conv4Channel.6'))


# ---- 4. the loss items on inputs that reach every branch ------------------------------------------------------------
LOSS_WEIGHTS = [(1, 1, 1, 1), (0.5, 2, 3, 0.25), (1, 1, 1, 0)]


def test_loss_items_on_every_branch(specs):
    """ffr_train_losses at N = 4 pairs on labels and encoder embeddings built from the float64 oracle's forward so that every
    branch runs: two of the four occluded rows are hits (accuracy exactly 0.5, not 0 == 0), two triplets are inactive and two
    active, the labels include the first and the last class, and the loss weights are not ones: the four items, the accuracy,
    and the gradients left in the handle (df_ext, dcos, extM) against the oracle's autograd cotangents."""
    import ffr_oracle_train as OT
    n = 4
    sd_r = synth.synth_state_dict(specs['recnet'], seed=0)
    g = torch.Generator().manual_seed(44)
    fm = torch.randn(2 * n, 512, 7, 7, generator=g) * 0.6
    eng = ffrnet_amd.Engine(0)
    f64 = dict(device=eng.device, dtype=torch.float64)
    with torch.no_grad():
        probe = OracleGraph(sd_r, fm, torch.zeros(n, dtype=torch.long), None, n, 2, **f64).outs
    f_new, cos = probe[0], probe[2]
    top2 = cos.topk(2, dim=1)
    assert (top2.values[:, 0] - top2.values[:, 1]).min().item() > 1e-4        # a condition on the seed: no near tie the GPU could break otherwise
    label = top2.indices[n:, 0].clone().cpu()                                 # rows 0, 1: the oracle's own choice for the occluded image
    label[2], label[3] = 0, 10574                                             # rows 2, 3: the first and the last class, both misses
    assert int(top2.indices[n + 2, 0]) != 0 and int(top2.indices[n + 3, 0]) != 10574
    f_enc = torch.randn(2 * n, 512, generator=g)
    f_enc[n:n + 2] = -f_new[n:n + 2].float().cpu()      # neg = 2: the hinge argument is near -0.9, inactive
    f_enc[n + 2:] = f_new[n + 2:].float().cpu()         # neg = 0: near 1.1, active
    # the oracle's forward with these labels; its outputs as leaves: the PARTIAL derivatives the handle keeps
    with torch.no_grad():
        outs = OracleGraph(sd_r, fm, label, None, n, 2, **f64).outs
    lab_d, fm_d, fe_d = label.to(eng.device), fm.to(**f64), f_enc.to(**f64)
    pos = 1 - torch.cosine_similarity(outs[0][n:], fe_d[:n])
    neg = 1 - torch.cosine_similarity(outs[0][n:], fe_d[n:])
    hinge = (pos - neg + 0.1).cpu()
    assert (hinge.abs() > 0.1).all() and (hinge[:2] < 0).all() and (hinge[2:] > 0).all(), hinge
    eng.train_init(sd_r)
    eng.train_forward(fm.cuda(), label.repeat(2).cuda(), groups=2, want=())
    for lw in LOSS_WEIGHTS:
        leaf = [o.clone().requires_grad_(True) for o in outs]
        items = OT.trainer_losses([o[:n] for o in leaf], [o[n:] for o in leaf], fm_d[:n], fe_d[:n], fe_d[n:], lab_d, loss_weight=lw)
        og = torch.autograd.grad(sum(items), leaf, allow_unused=True)
        og = [v if v is not None else torch.zeros_like(o) for v, o in zip(og, leaf)]
        out5 = eng.train_losses(f_enc.cuda(), loss_weight=lw).cpu()
        want = [float(i.detach()) for i in items]
        print(lw, out5.tolist(), want)
        assert np.allclose(out5[:4].numpy(), want, rtol=1e-4), (lw, out5, want)
        assert float(out5[4]) == 0.5, (lw, out5)
        df = eng.train_debug('df_ext', (2 * n, 512))
        assert rel(df, og[0]) < 1e-4, (lw, rel(df, og[0]))
        # an inactive triplet leaves the identity term alone: 2 lw2 / (2 N 512) (f_new - f_enc_non)
        ident = (lw[2] / (n * 512.0)) * (outs[0][n:n + 2] - fe_d[:2])
        assert rel(df[n:n + 2], ident) < 1e-4, (lw, rel(df[n:n + 2], ident))
        dcos = eng.train_debug('dcos', (2 * n, 10624))
        assert rel(dcos[:, :10575], 30.0 * og[1]) < 1e-4, (lw, rel(dcos[:, :10575], 30.0 * og[1]))
        assert torch.equal(dcos[:, 10575:], torch.zeros(2 * n, 49)), lw
        if lw[3] == 0:
            assert torch.equal(dcos, torch.zeros_like(dcos)), lw
        else:
            assert dcos.abs().max() > 0
        ext = eng.train_debug('extM', (2 * n * 49, 1024)).reshape(2 * n, 49, 1024)
        d_fs = og[5].reshape(2 * n, 512, 49).permute(0, 2, 1)
        d_fc = og[6].reshape(2 * n, 512, 49).permute(0, 2, 1)
        assert rel(ext[:, :, :512], d_fs) < 2e-4, (lw, rel(ext[:, :, :512], d_fs))
        assert rel(ext[:, :, 512:], d_fc) < 2e-4, (lw, rel(ext[:, :, 512:], d_fc))


# ---- 5. loss gradients, slots and scratch: wrong must be loud -------------------------------------------------------
class Slots(object):
    """Fixed feature maps of 2 x 2 ('a', 'a2') and 2 x 3 ('b') images, labels, embeddings and cotangents; handles that run
    direct convolutions.  Every sequence is compared, bit for bit on the flat gradient buffer, with a fresh handle that ran
    only the intended part of it."""

    def __init__(self, specs):
        self.sd_r = synth.synth_state_dict(specs['recnet'], seed=0)
        g = torch.Generator().manual_seed(71)
        self.fm, self.label, self.f_enc, self.cots = {}, {}, {}, {}
        for tag, n in (('a', 2), ('a2', 2), ('b', 3)):
            self.fm[tag] = (torch.randn(2 * n, 512, 7, 7, generator=g) * 0.6).cuda()
            self.label[tag] = torch.randint(0, 10575, (n,), generator=g).repeat(2).cuda()
            self.f_enc[tag] = torch.randn(2 * n, 512, generator=g).cuda()
            self.cots[tag] = [(torch.randn(2 * n, 512, generator=g) * 1e-2).cuda(), None, None, (torch.randn(2 * n, 49, 49, generator=g) * 1e-2).cuda(),
                              (torch.randn(2 * n, 512, 512, generator=g) * 1e-3).cuda(), None, None]

    def handle(self):
        eng = ffrnet_amd.Engine(0)
        eng.train_init(self.sd_r)
        eng.train_option('winograd', 0)
        info = eng.train_info()
        return eng, torch.as_tensor(FlatBuffer(info['grads'], info['n_flat']), device=eng.device)

    def forward(self, eng, tag, slot):
        eng.train_forward(self.fm[tag], self.label[tag], groups=2, slot=slot, want=())

    def backward(self, eng, flat, tag, slot):
        eng.train_zero_grad()
        eng.train_backward(self.cots[tag], slot=slot)
        torch.cuda.synchronize()
        return flat.clone()

    def fresh(self, tag, losses=False, fold=1):
        """The bits of a handle that only ever ran forward + backward (or + losses + backward_losses) of `tag`, in slot 0."""
        eng, flat = self.handle()
        eng.train_option('fold_channel', fold)
        self.forward(eng, tag, 0)
        if not losses:
            return self.backward(eng, flat, tag, 0)
        eng.train_losses(self.f_enc[tag], slot=0)
        eng.train_zero_grad()
        eng.train_backward_losses(slot=0)
        torch.cuda.synchronize()
        return flat.clone()


@pytest.fixture(scope='module')
def slots(specs):
    return Slots(specs)


def refused(eng, flat, slot):
    """train_backward_losses(slot) fails with FFR_ERR_STATE (-2) and leaves the gradient buffer as it was."""
    eng.train_zero_grad()
    flat.fill_(0.25)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='native error -2'):
        eng.train_backward_losses(slot=slot)
    torch.cuda.synchronize()
    assert torch.equal(flat, torch.full_like(flat, 0.25))


@pytest.mark.parametrize('order', [(0, 1), (1, 0)])
def test_two_slots_and_a_scratch_that_regrows_between(slots, order):
    """Forward of 2 x 2 images into slot 0, of 2 x 3 into slot 1 (the shared backward scratch is reallocated for it), then both
    backwards in either order: each gives the bits of a fresh handle that ran it alone."""
    want = {0: slots.fresh('a'), 1: slots.fresh('b')}
    eng, flat = slots.handle()
    slots.forward(eng, 'a', 0)
    slots.forward(eng, 'b', 1)
    for slot in order:
        got = slots.backward(eng, flat, 'ab'[slot], slot)
        assert got.abs().max() > 0 and torch.equal(got, want[slot]), (order, slot, (got - want[slot]).abs().max().item())


def test_loss_gradients_belong_to_their_slot(slots):
    """train_losses(slot 0), train_backward_losses(slot 1) with a valid forward in both: the gradients in the handle are those of
    slot 0's forward, so slot 1 is refused -- and slot 0 still gets them."""
    eng, flat = slots.handle()
    slots.forward(eng, 'a', 0)
    slots.forward(eng, 'a2', 1)
    eng.train_losses(slots.f_enc['a'], slot=0)
    refused(eng, flat, 1)
    eng.train_zero_grad()
    eng.train_backward_losses(slot=0)
    torch.cuda.synchronize()
    assert torch.equal(flat, slots.fresh('a', losses=True))


def test_loss_gradients_end_when_the_scratch_regrows(slots):
    """train_losses(slot 0), then a forward of more images into slot 1: the scratch that held the loss gradients is freed and
    a zeroed one takes its place."""
    eng, flat = slots.handle()
    slots.forward(eng, 'a', 0)
    eng.train_losses(slots.f_enc['a'], slot=0)
    slots.forward(eng, 'b', 1)
    refused(eng, flat, 0)


def test_loss_gradients_end_at_another_backward(slots):
    """train_losses(slot 0), then forward + backward with explicit cotangents in slot 1, which overwrites dcos and extM."""
    eng, flat = slots.handle()
    slots.forward(eng, 'a', 0)
    slots.forward(eng, 'a2', 1)
    eng.train_losses(slots.f_enc['a'], slot=0)
    slots.backward(eng, flat, 'a2', 1)
    refused(eng, flat, 0)


def test_loss_gradients_end_at_a_new_forward_in_their_slot(slots):
    """train_losses(slot 0), then another forward into slot 0: the gradients were those of the forward it replaced."""
    eng, flat = slots.handle()
    slots.forward(eng, 'a', 0)
    eng.train_losses(slots.f_enc['a'], slot=0)
    slots.forward(eng, 'a2', 0)
    refused(eng, flat, 0)


def test_folded_products_survive_a_regrown_scratch(slots):
    """A folded forward in slot 0, then fold_channel = 0 and a larger forward in slot 1: the scratch that held the folded 32x32
    products is reallocated and nothing writes them again before slot 0's backward, which forms them anew from the live weights
    and gives the bits of a fresh handle."""
    want = slots.fresh('a')
    eng, flat = slots.handle()
    slots.forward(eng, 'a', 0)
    eng.train_option('fold_channel', 0)
    slots.forward(eng, 'b', 1)
    got = slots.backward(eng, flat, 'a', 0)
    assert sorted(fold_names(eng.train_wgrad_plan())) == ['Conv4Channel.fold0', 'Conv4Channel.fold1']
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert torch.equal(slots.backward(eng, flat, 'b', 1), slots.fresh('b', fold=0))
