"""Test infrastructure: plain restatements of the four RecNet operators of csrc/recnet_ops.hip (reference models/recnet.py:
220-236 selfSimilarity, 372-386 Conv4Channel, 398-423 forward), written with matmul / where / exp only and evaluated in the
dtype of their input -- float64 is the reference of tests/test_gpu_recnet_ops.py, float32 its yardstick for what fp32
costs.  Nothing is folded or re-associated: ss_channel and M_channel are formed in full, the six linears of Conv4Channel run one
after the other.  tests/test_host_recnet_ops.py pins them to the float64 run of oracle/ffr_oracle.py."""
import torch

EPS = 1e-12          # F.normalize's eps: v / max(|v|, eps)
LINEARS = ((0, 1), (2, None), (3, 4), (5, None), (6, 7), (8, None))      # Conv4Channel: (Linear, the PReLU after it)
FAMILIES = ('seed0', 'trained', 'kaiming')


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def ss_space(x):
    """[N,512,7,7] -> [N,49,49]: cosine of the position vectors (over the 512 channels)."""
    v = x.reshape(x.size(0), x.size(1), -1)                         # [N, C, P]
    norm = (v * v).sum(1).sqrt().clamp_min(EPS)                     # [N, P]
    u = v / norm[:, None, :]
    return torch.matmul(u.transpose(1, 2), u)


def ss_channel(x):
    """[N,512,7,7] -> [N,512,512]: cosine of the channel vectors (over the 49 positions)."""
    v = x.reshape(x.size(0), x.size(1), -1)
    norm = (v * v).sum(2).sqrt().clamp_min(EPS)                     # [N, C]
    u = v / norm[:, :, None]
    return torch.matmul(u, u.transpose(1, 2))


def m_channel(x, sd):
    """sigmoid(Conv4Channel([X_c | ss_channel_c])) -> [N,512,512]; the PReLU(512) slopes belong to the 512 rows."""
    v = x.reshape(x.size(0), x.size(1), -1)
    z = torch.cat((v, ss_channel(x)), 2)                            # [N, 512, 49 + 512]
    for lin, act in LINEARS:
        z = torch.matmul(z, sd['Conv4Channel.%d.weight' % lin].t()) + sd['Conv4Channel.%d.bias' % lin]
        if act is not None:
            slope = sd['Conv4Channel.%d.func.weight' % act]
            z = torch.where(z >= 0, z, z * slope[None, :, None])
    return 1.0 / (1.0 + torch.exp(-z))


def apply_channel(M, x):
    """feat_channel_raw = M_channel @ X -> [N,512,7,7]"""
    return torch.matmul(M, x.reshape(x.size(0), x.size(1), -1)).reshape(x.shape)


def feat_channel_raw(x, sd):
    return apply_channel(m_channel(x, sd), x)


def feat_space(x, M_space):
    """X @ M_space -> [N,512,7,7], M_space [N,49,49]"""
    return torch.matmul(x.reshape(x.size(0), x.size(1), -1), M_space).reshape(x.shape)


def mean7x7(feat):
    """[N,C,7,7] -> [N,C]"""
    return feat.reshape(feat.size(0), feat.size(1), -1).sum(2) / 49.0


def edit_featmaps(fm):
    """The edge cases of the operator tests on a copy of three featmaps [3,512,7,7]: image 0 keeps its values but for one
    channel scaled to 1e-20 (its norm is below the 1e-12 clamp); image 1 has one zero channel and one zero position; image 2 is
    all zero (every norm is clamped, ss_* are 0, M_channel comes from the biases alone)."""
    assert tuple(fm.shape) == (3, 512, 7, 7)
    fm = fm.clone()
    fm[0, 301] *= 1e-20
    fm[1, 77] = 0.0
    fm[1, :, 3, 5] = 0.0
    fm[2] = 0.0
    return fm


def weight_sets(specs, golden_dir):
    """{family: (encoder state_dict, RecNet state_dict)}: the seed-0 synthetic set and the 'trained' / 'kaiming' families of
    golden G11."""
    from ffrnet_amd import synth
    out = {'seed0': (synth.synth_state_dict(specs['encoder'], seed=0), synth.synth_state_dict(specs['recnet'], seed=0))}
    for name in ('trained', 'kaiming'):
        out[name] = synth.stress_state_dicts(name, specs['encoder'], specs['recnet'], golden_dir)
    return out


def err(a, ref):
    """max-abs error over the reference's abs-max (0 over 0 counts as 0: an all-zero reference asks for exact zeros)"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    d = (a - ref).abs().max().item()
    if d != d:
        return float('inf')
    return 0.0 if d == 0.0 else d / max(ref.abs().max().item(), 1e-300)
