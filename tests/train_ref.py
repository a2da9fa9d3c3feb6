"""What the tests of the RecNet training step share (tests/test_gpu_train.py, tests/test_gpu_train_cotangents.py,
tests/test_host_train_ref.py): error measures, the PReLU-kink transplant, and the oracle's parameter gradients
(oracle/ffr_oracle_train.py under torch autograd) for the Trainer's loss or for any cotangents of the seven outputs.
Plain module: nothing here needs a GPU unless it is handed an Engine."""
import os
import sys

import torch
import torch.nn.functional as F

from ffrnet_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

NAMES = ['f_new', 'pred_loss', 'pred_label', 'M_space', 'M_channel', 'feat_space', 'feat_channel']


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def grad_err(got, ref):
    # a BatchNorm bias in front of [identity -> conv -> BatchNorm] has a gradient that is zero up to rounding
    # (the next BatchNorm removes the shift): errors are taken relative to at least 1e-3
    return ((got.double().cpu() - ref.double()).abs().max() / max(ref.abs().max().item(), 1e-3)).item()


# ---- PReLU kinks ------------------------------------------------------------------------------------------
# RecNet has 2.1 M PReLU inputs in an 8-image step; a forward that differs from the reference's by 1e-5 (F(4x4,3x3) in fp32,
# another encoder) puts a few dozen of them on the other side of zero, and each such element changes its own gradient by
# (1 - slope) -- percents of a parameter gradient's norm, although NOTHING is wrong (the oracle does the same to itself:
# a 1e-5 relative perturbation of its float64 inputs moves its own gradients by 7e-3..1e-2 in relative L2, a 1e-6 one by
# 3e-6; tools/train_grad_report.py).  The reference-pinned check of a gradient therefore takes the SIGN PATTERN the GPU
# forward produced (ffr_train_debug_copy: y * scale + shift per ConvLayer, the three row pre-activations of
# Conv4Channel), evaluates the oracle's gradient formula on THAT side of every kink (ffr_oracle_train._prelu, ctl['mask']),
# and (a) holds the GPU gradients to it tightly, per tensor, in the default (Winograd) arithmetic and with the real slopes;
# (b) requires every element whose side differs from the oracle's own to lie within the forward tolerance of zero -- the
# only place where two correct fp32 forwards may disagree.
def gpu_kink_masks(eng, groups, n, slot=0):
    """{oracle PReLU name: [groups * n, ...] bool, True = the identity side} of the forward held in `slot`."""
    import ffr_oracle_train as OT
    imgs = groups * n
    masks = {}
    for name, dbg in OT.PRELU_LAYERS:
        if dbg.startswith('h'):
            masks[name] = eng.train_debug(dbg, (imgs * 512, 64), slot)[:, :32].reshape(imgs, 512, 32) > 0
            continue
        c = {'sp': (256, 256, 256, 128, 128, 128, 49, 49, 49), 'fm': (512,) * 3, 'mg': (512,) * 3}[dbg[:2]][int(dbg[2])]
        cp = (c + 63) // 64 * 64
        y = eng.train_debug('y.' + dbg, (groups, n * 49, cp), slot).double()
        sc = eng.train_debug('scale.' + dbg, (groups, 1, cp), slot).double()
        sh = eng.train_debug('shift.' + dbg, (groups, 1, cp), slot).double()
        z = (y * sc + sh).reshape(imgs, 7, 7, cp)[..., :c].permute(0, 3, 1, 2)      # the kernel's fma, exactly (float64 holds the product)
        masks[name] = z > 0
    return masks


def check_kinks(masks, pre, tol):
    """Every element whose side differs from the oracle's own lies within `tol` (relative to its layer's largest
    pre-activation) of zero.  -> number of such elements."""
    flipped = 0
    for k, m in masks.items():
        nat = pre[k]
        diff = m != (nat > 0)
        if diff.any():
            margin = (nat[diff].abs().max() / nat.abs().max()).item()
            assert margin < tol, (k, int(diff.sum()), margin)
            flipped += int(diff.sum())
    return flipped


def oracle_grads_on_masks(sd_r, fm, f_enc, label, masks, n, device='cpu', dtype=torch.float32):
    """The oracle's parameter gradients of Trainer.backward's loss with every PReLU element on the side `masks` says
    (None: its own side).  fm / f_enc: [2 n, ...] clean then occluded.  Evaluated on `device` in `dtype` (weights, feature
    maps, embeddings converted).  -> ({key: grad}, natural pre-activations, items), tensors on `device`"""
    import ffr_oracle_train as OT
    keys = OT.trainable_keys(sd_r)
    conv = dict(device=device, dtype=dtype)
    fm, f_enc, label = fm.to(**conv), f_enc.to(**conv), label.to(device)
    masks = {k: m.to(device) for k, m in masks.items()} if masks else masks
    params = {k: sd_r[k].to(**conv, copy=True).requires_grad_(True) for k in keys}
    running = {k: v.to(**conv, copy=True) if v.is_floating_point() else v.to(device, copy=True) for k, v in sd_r.items()
               if k not in params}
    ctl = [{'mask': {k: m[:n] for k, m in masks.items()}} if masks else {}, {'mask': {k: m[n:] for k, m in masks.items()}} if masks else {}]
    out_non = OT.recnet_train_forward(params, fm[:n], label, running, ctl[0])
    out_ocl = OT.recnet_train_forward(params, fm[n:], label, running, ctl[1])
    items = OT.trainer_losses(out_non, out_ocl, fm[:n], f_enc[:n], f_enc[n:], label)
    grads = torch.autograd.grad(sum(items), [params[k] for k in keys], allow_unused=True)
    pre = {k: torch.cat([ctl[0]['pre'][k], ctl[1]['pre'][k]]) for k in ctl[0]['pre']}
    return {k: (g if g is not None else torch.zeros_like(params[k])) for k, g in zip(keys, grads)}, pre, [float(i.detach()) for i in items]


class OracleGraph(object):
    """oracle_grads_on_masks for ANY loss that is linear in the seven outputs: the oracle's train-mode forward of `groups`
    BatchNorm batches of n images (fm [groups * n, 512, 7, 7], label [n], shared by the groups as the Trainer shares it, or
    [groups * n]) with every PReLU element on the side `masks` says (None: its own), built ONCE; grads(cots) then differentiates
    sum_i <out_i, cot_i> through it, once per set of cotangents.  Evaluated on `device` in `dtype`.
      outs   the seven outputs, groups stacked along dim 0, in the shapes of Engine.train_forward (detached)
      pre    {PReLU name: pre-activation}, groups stacked (with masks=None: the natural ones check_kinks wants)
      t2     Conv4Channel's first 512-wide intermediate, the output of Conv4Channel.2, [groups * n, 512, 512]"""

    def __init__(self, sd_r, fm, label, masks, n, groups=2, device='cpu', dtype=torch.float64):
        import ffr_oracle_train as OT
        assert fm.size(0) == groups * n and label.numel() in (n, groups * n)
        self.keys = OT.trainable_keys(sd_r)
        conv = dict(device=device, dtype=dtype)
        fm, label = fm.to(**conv), label.to(device)
        label = label.repeat(groups) if label.numel() == n else label
        self.params = {k: sd_r[k].to(**conv, copy=True).requires_grad_(True) for k in self.keys}
        running = {k: v.to(**conv, copy=True) if v.is_floating_point() else v.to(device, copy=True) for k, v in sd_r.items()
                   if k not in self.params}
        per_group, ctls = [], []
        for g in range(groups):
            part = slice(g * n, (g + 1) * n)
            ctl = {'mask': {k: m[part].to(device) for k, m in masks.items()}} if masks else {}
            per_group.append(OT.recnet_train_forward(self.params, fm[part], label[part], running, ctl))
            ctls.append(ctl)
        imgs = groups * n
        shapes = [(imgs, 512), (imgs, 10575), (imgs, 10575), (imgs, 49, 49), (imgs, 512, 512), (imgs, 512, 7, 7), (imgs, 512, 7, 7)]
        self._outs = [torch.cat([o[i] for o in per_group]).reshape(s) for i, s in enumerate(shapes)]
        self.outs = [o.detach() for o in self._outs]
        self.pre = {k: torch.cat([c['pre'][k] for c in ctls]) for k in ctls[0]['pre']}
        self.device, self.dtype = device, dtype
        with torch.no_grad():
            import ffr_oracle as fo
            p = self.params
            x = torch.cat((fm.reshape(imgs, 512, -1), fo.self_similarity(fm)[1]), 2)
            z = F.linear(x, p['Conv4Channel.0.weight'], p['Conv4Channel.0.bias'])
            slope = p['Conv4Channel.1.func.weight']
            h1 = torch.where(masks['Conv4Channel.1'].to(device), z, z * slope.view(1, -1, 1)) if masks else F.prelu(z, slope)
            self.t2 = F.linear(h1, p['Conv4Channel.2.weight'], p['Conv4Channel.2.bias']).detach()

    def grads(self, cots):
        """cots: seven tensors in the shapes of `outs`, or None (no such term).  -> {key: gradient, or None where no path leads
        from the chosen outputs to the parameter}: the caller needs to know which those are, so they are not zeros."""
        assert len(cots) == 7
        loss = sum((o * c.to(device=self.device, dtype=self.dtype)).sum() for o, c in zip(self._outs, cots) if c is not None)
        g = torch.autograd.grad(loss, [self.params[k] for k in self.keys], allow_unused=True, retain_graph=True)
        return dict(zip(self.keys, g))


def stack_trainer_cotangents(tc):
    """build_train_case's 14 output cotangents (clean 7-tuple, occluded 7-tuple) as seven stacked ones (None: no path)."""
    og, stacked = tc['out_grads'], []
    for i in range(7):
        a, b = og[i], og[7 + i]
        if a is None and b is None:
            stacked.append(None)
            continue
        shp = tc['out_non'][i].shape
        stacked.append(torch.cat([a if a is not None else torch.zeros(shp), b if b is not None else torch.zeros(shp)]))
    return stacked


def build_train_case(specs, smooth=False, family=None):
    """The G8 scenario (4 clean + 4 occluded images, synthetic weights; `family`: the weights of golden G12 instead) through
    the ORACLE with autograd: outputs, gradients wrt the seven outputs of both RecNet calls, parameter gradients (unclipped)."""
    import ffr_oracle as O
    import ffr_oracle_train as OT
    if family:
        sd_e, sd_r = synth.stress_state_dicts(family, specs['encoder'], specs['recnet'], os.path.join(ROOT, 'tests', 'golden'))
    else:
        sd_e = synth.synth_state_dict(specs['encoder'], seed=0)
        sd_r = synth.synth_state_dict(specs['recnet'], seed=0)
    if smooth:      # PReLU slopes of 1: the network has no kinks, gradients are continuous in every rounding
        for k in sd_r:
            if k.endswith('func.weight'):
                sd_r[k] = torch.ones_like(sd_r[k])
    non, ocl, label = synth.synth_train_batch(4, seed=301)
    with torch.no_grad():
        fm_non, fe_non = O.encoder_forward(sd_e, non)
        fm_ocl, fe_ocl = O.encoder_forward(sd_e, ocl)
    keys = OT.trainable_keys(sd_r)
    params = {k: sd_r[k].clone().requires_grad_(True) for k in keys}
    running = {k: v.clone() for k, v in sd_r.items() if k not in params}
    out_non = OT.recnet_train_forward(params, fm_non, label, running)
    out_ocl = OT.recnet_train_forward(params, fm_ocl, label, running)
    items = OT.trainer_losses(out_non, out_ocl, fm_non, fe_non, fe_ocl, label)
    grads = torch.autograd.grad(sum(items), [params[k] for k in keys], allow_unused=True)
    pg = {k: (g if g is not None else torch.zeros_like(params[k])) for k, g in zip(keys, grads)}
    # cotangents of the 7-tuples: the PARTIAL derivatives of the loss, outputs taken as independent leaves
    # (pred_loss is a function of pred_label, f_new of feat_space ... inside the graph)
    leaf_non = [o.detach().clone().requires_grad_(True) for o in out_non]
    leaf_ocl = [o.detach().clone().requires_grad_(True) for o in out_ocl]
    items_l = OT.trainer_losses(leaf_non, leaf_ocl, fm_non, fe_non, fe_ocl, label)
    og = torch.autograd.grad(sum(items_l), leaf_non + leaf_ocl, allow_unused=True)
    return dict(sd_r=sd_r, f_enc=torch.cat([fe_non, fe_ocl]), fm=torch.cat([fm_non, fm_ocl]), label=torch.cat([label, label]), out_non=out_non,
                out_ocl=out_ocl, out_grads=og, param_grads=pg, running=running, keys=keys,
                losses=[float(l.detach()) for l in items])
