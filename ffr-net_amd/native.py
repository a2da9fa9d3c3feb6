"""ctypes binding of libffrnet_hip.so (include/ffrnet.h).

PyTorch is used for device memory and streams only: tensors are handed over as raw
device pointers (`tensor.data_ptr()`) and launches go to torch's current HIP stream.
"""
import ctypes as C
import os

import torch

from . import align as _align

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

KCLASS_NAMES = ['conv_igemm', 'stem', 'se', 'combine', 'head', 'selfsim', 'channel',
                'space', 'layout', 'score', 'wino', 'wino_fused', 'wgrad',
                'train_bn', 'train_loss', 'train_optim', 'train_xform', 'train_elem']


class NativeLibraryMissing(RuntimeError):
    pass


class TensorDesc(C.Structure):
    _fields_ = [('name', C.c_char_p), ('data', C.c_void_p), ('ndim', C.c_int32),
                ('shape', C.c_int64 * 4)]


class MemStats(C.Structure):
    _fields_ = [('encoder_weight_bytes', C.c_size_t), ('recnet_weight_bytes', C.c_size_t), ('mixed_tile_weight_bytes', C.c_size_t),
                ('workspace_bytes', C.c_size_t), ('encoder_load_seconds', C.c_double), ('recnet_load_seconds', C.c_double),
                ('mixed_tile_pack_seconds', C.c_double), ('split_weight_bytes', C.c_size_t),
                ('wf_split_weight_bytes', C.c_size_t), ('wf_split_launches', C.c_longlong)]


class KClassStat(C.Structure):
    _fields_ = [('launches', C.c_int64), ('ms', C.c_double), ('flops', C.c_double),
                ('bytes', C.c_double), ('flops_executed', C.c_double), ('flops_useful', C.c_double)]


class ConvDesc(C.Structure):
    _fields_ = [('x', C.c_void_p), ('N', C.c_int), ('H', C.c_int), ('W', C.c_int),
                ('in_pitch', C.c_int), ('cin_pad', C.c_int),
                ('w', C.c_void_p), ('bias', C.c_void_p), ('slope', C.c_void_p),
                ('resid', C.c_void_p), ('res_pitch', C.c_int),
                ('out', C.c_void_p), ('out_pitch', C.c_int), ('out_coff', C.c_int),
                ('cout_store', C.c_int), ('cout_pad', C.c_int),
                ('R', C.c_int), ('S', C.c_int), ('stride', C.c_int), ('pad', C.c_int),
                ('pad_mode', C.c_int), ('border_bias', C.c_int), ('flags', C.c_int),
                ('tile', C.c_int), ('splitk', C.c_int)]


class LayerInfo(C.Structure):
    _fields_ = [('name', C.c_char * 64), ('net', C.c_int), ('arith', C.c_int), ('sensitivity', C.c_double)]


class WgradLaunch(C.Structure):
    _fields_ = [('name', C.c_char * 48)] + [(f, C.c_int) for f in (
        'path', 'rows', 'cout_pad', 'Ng', 'nbatch', 'nkt', 'splits', 'kt_per_split', 'full_tiles', 'tail_splits', 'tail_kt',
        'accumulate')]


class Conv3x3Desc(C.Structure):
    _fields_ = [('x', C.c_void_p), ('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('cin', C.c_int), ('in_pitch', C.c_int),
                ('w_host', C.c_void_p), ('bias_host', C.c_void_p), ('slope_host', C.c_void_p), ('cout', C.c_int),
                ('in_scale_host', C.c_void_p), ('in_shift_host', C.c_void_p),
                ('resid', C.c_void_p), ('res_pitch', C.c_int),
                ('out', C.c_void_p), ('out_pitch', C.c_int), ('out_coff', C.c_int), ('cout_store', C.c_int),
                ('pad_mode', C.c_int), ('use_wino', C.c_int), ('flags', C.c_int),
                ('tile_sums', C.c_void_p)]


class ConvLaunch(C.Structure):
    _fields_ = [(f, C.c_int) for f in ('path', 'images', 'rows', 'tile', 'nblocks', 'granule', 'nkt', 'tiles', 'cut', 'split',
                                       'phased', 'half_n', 'block_tiles', 'n_main', 'side', 'stride', 'conv_shortcut', 'se_scale')]


CONV_PATHS = ('direct', 'fused', 'unfused-gemm-stream', 'unfused-igemm', 'mixed', 'tail-split', 'channel', 'se-pool', 'se-tiles',
              'combine', 'combine-in-c', 'combine-in-mixed', 'wino-out-in')
WGRAD_PATHS = ('plain-taps9', 'plain-taps1', 'batched')
ARITH = {'direct': 0, 'winograd': 1}
CALIB_TENSORS = ('f', 'featmap', 'f_new', 'feat_new')


_LIB_PATH = os.path.join(_HERE, 'libffrnet_hip.so')


def lib_path():
    return _LIB_PATH


def set_library(path):
    """Use another build of the library (tools/trace_build.py: the -DFFR_TRACE diagnostics build).  Must be called
    before the first Engine is created; the product never calls it."""
    global _LIB_PATH
    if _LIB is not None:
        raise RuntimeError('ffrnet_amd: the native library is already loaded')
    _LIB_PATH = os.path.abspath(path)


# every symbol include/ffrnet.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ('ffr_create', C.c_int, [C.POINTER(_P), C.c_int]),
    ('ffr_destroy', None, [_P]),
    ('ffr_last_error', C.c_char_p, [_P]),
    ('ffr_version', C.c_char_p, []),
    ('ffr_load_encoder', C.c_int, [_P, C.POINTER(TensorDesc), C.c_int]),
    ('ffr_load_recnet', C.c_int, [_P, C.POINTER(TensorDesc), C.c_int]),
    ('ffr_encoder_forward', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ('ffr_recnet_forward', C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    ('ffr_embed', C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    ('ffr_embed_u8', C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P]),
    ('ffr_encoder_forward_u8', C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ('ffr_cosine_scores', C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    ('ffr_lfw_fold_accuracy', C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, _P]),
    ('ffr_row_norms', C.c_int, [_P, _P, C.c_longlong, C.c_int, _P, _P]),
    ('ffr_search_topk', C.c_int, [_P, _P, C.c_int, _P, _P, C.c_longlong, C.c_int, C.c_int, C.c_longlong, _P, _P, _P]),
    ('ffr_topk_merge', C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ('ffr_search_topk_subjects', C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.c_int, _P, _P, _P,
                                           _P]),
    ('ffr_search_topk_filtered', C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, _P, C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.c_int, _P,
                                           _P, _P, _P]),
    ('ffr_topk_merge_subjects', C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    ('ffr_coarse_pack', C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, _P, _P, _P]),
    ('ffr_search_topk_coarse', C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.c_longlong, C.c_int, C.c_int, C.c_longlong, _P, _P, _P, _P]),
    ('ffr_search_topk_coarse_subjects', C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P, C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.c_int,
                                                  _P, _P, _P, _P, _P]),
    ('ffr_search_topk_coarse_filtered', C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_longlong, C.c_int, C.c_int, C.c_longlong,
                                                  C.c_int, _P, _P, _P, _P, _P]),
    ('ffr_cluster_threshold', C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, C.c_float, _P, _P]),
    ('ffr_cluster_templates', C.c_int, [_P, _P, _P, _P, _P, C.c_longlong, C.c_int, _P, _P]),
    ('ffr_cluster_extend', C.c_int, [_P, _P, _P, C.c_longlong, C.c_longlong, C.c_int, C.c_float, _P, _P, _P]),
    ('ffr_cluster_remove', C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, C.c_float, _P, _P, _P, _P, _P]),
    ('ffr_cluster_density', C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P]),
    ('ffr_cluster_density_extend', C.c_int, [_P, _P, _P, C.c_longlong, C.c_longlong, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P, _P]),
    ('ffr_cluster_density_remove', C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P, _P, _P]),
    ('ffr_align_transforms', C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, _P]),
    ('ffr_align_warp', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_longlong, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    ('ffr_embed_aligned', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_longlong, _P, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P,
                                    _P]),
    ('ffr_workspace_bytes', C.c_size_t, [_P, C.c_int, C.c_int, C.c_int]),
    ('ffr_reserve', C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    ('ffr_generation', C.c_ulonglong, [_P]),
    ('ffr_layer_count', C.c_int, [_P, C.POINTER(C.c_int)]),
    ('ffr_layer_get', C.c_int, [_P, C.c_int, C.POINTER(LayerInfo)]),
    ('ffr_layer_set_arith', C.c_int, [_P, C.c_int, C.c_int]),
    ('ffr_calibrate', C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), _P]),
    ('ffr_memory_stats', C.c_int, [_P, _P]),
    ('ffr_split_planes_host', C.c_int, [_P, C.c_longlong, _P]),
    ('ffr_set_option', C.c_int, [_P, C.c_char_p, C.c_longlong]),
    ('ffr_get_option', C.c_int, [_P, C.c_char_p, C.POINTER(C.c_longlong)]),
    ('ffr_probe_mfma_peak', C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    ('ffr_profile_enable', C.c_int, [_P, C.c_int]),
    ('ffr_profile_read', C.c_int, [_P, C.POINTER(KClassStat)]),
    ('ffr_op_conv', C.c_int, [_P, C.POINTER(ConvDesc), _P]),
    ('ffr_op_conv3x3', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ('ffr_op_conv3x3_ex', C.c_int, [_P, C.POINTER(Conv3x3Desc), _P]),
    ('ffr_conv_plan_record', C.c_int, [_P, C.c_int]),
    ('ffr_conv_plan_read', C.c_int, [_P, C.POINTER(ConvLaunch), C.c_int, C.POINTER(C.c_int)]),
    ('ffr_plan_igemm_host', C.c_int, [C.c_longlong] + [C.c_int] * 7 + [_P, _P, _P]),
    ('ffr_plan_conv_host', C.c_int, [C.c_int] * 20 + [_P]),
    ('ffr_encoder_trunk_nhwc', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    ('ffr_plan_channel_rows_host', C.c_int, [C.c_int, C.c_int, C.c_int, _P]),
    ('ffr_recnet_debug', C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P]),
    # include/ffrnet_train.h
    ('ffr_op_convlayer_train', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ('ffr_train_init', C.c_int, [_P, C.POINTER(TensorDesc), C.c_int]),
    ('ffr_train_info', C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_longlong),
                                 C.POINTER(C.c_int)]),
    ('ffr_train_get', C.c_int, [_P, C.c_int, C.c_char_p, _P, C.c_size_t]),
    ('ffr_train_set', C.c_int, [_P, C.c_int, C.c_char_p, _P, C.c_size_t]),
    ('ffr_train_zero_grad', C.c_int, [_P, _P]),
    ('ffr_train_forward', C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    ('ffr_train_backward', C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    ('ffr_train_adam_step', C.c_int, [_P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P]),
    ('ffr_train_debug_copy', C.c_int, [_P, C.c_int, C.c_char_p, _P, C.c_size_t]),
    ('ffr_train_option', C.c_int, [_P, C.c_char_p, C.c_int]),
    ('ffr_train_wgrad_plan', C.c_int, [_P, C.POINTER(WgradLaunch), C.c_int, C.POINTER(C.c_int)]),
    ('ffr_train_buckets', C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    ('ffr_train_bucket_wait', C.c_int, [_P, C.c_int, _P]),
    ('ffr_train_export', C.c_int, [_P, C.c_int, C.c_char_p, _P, _P]),
    ('ffr_train_import', C.c_int, [_P, C.c_int, C.c_char_p, _P, _P]),
    ('ffr_train_losses', C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_double), _P, _P]),
    ('ffr_train_backward_losses', C.c_int, [_P, C.c_int, _P]),
    ('ffr_train_iteration', C.c_int, [_P, _P, _P, _P, C.c_int, C.POINTER(C.c_double), _P, _P]),
    ('ffr_train_iteration_u8', C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_double), _P, _P]),
]


def load_library():
    """dlopen the in-tree library once; no fallback of any kind."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise NativeLibraryMissing(
            'ffrnet_amd: %s not found -- build it with `python -c "import __graft_entry__ as g; '
            'g.build()"` (hipcc --offload-arch=gfx950). There is no CPU fallback.' % path)
    lib = C.CDLL(path)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the library lacks a symbol
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _check(t, name, device, dtype=torch.float32, shape=None, hint=''):
    """Boundary check of a tensor handed to the library as a raw pointer: a torch.Tensor on `device` (the handle's; None
    skips that one question) of `dtype`, and of `shape` when given -- one entry per dimension, a string standing for any
    size.  A tensor on ANOTHER GPU is rejected: its pointer would be dereferenced by kernels running on the handle's GPU
    (peer reads over xGMI at best, a fault at worst)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('ffrnet_amd: %s is on %s; the native HIP path needs a ROCm device '
                           'tensor (there is no CPU fallback)' % (name, t.device))
    if device is not None and t.device.index != device.index:
        raise RuntimeError('ffrnet_amd: %s is on %s but this Engine lives on %s; move the tensor there (or create the '
                           'Engine on the tensor\'s device: one process per GPU calls torch.cuda.set_device(local_rank) '
                           'before anything else)' % (name, t.device, device))
    if t.dtype != dtype:
        raise RuntimeError('ffrnet_amd: %s must be %s, got %s' % (name, str(dtype).replace('torch.', ''), t.dtype))
    if shape is not None and (len(t.shape) != len(shape) or
                              any(not isinstance(want, str) and got != want for got, want in zip(t.shape, shape))):
        raise RuntimeError('ffrnet_amd: %s expected shape [%s]%s, got %s'
                           % (name, ','.join(map(str, shape)), hint, list(t.shape)))


def _check_dev(t, name, shape_tail=None, device=None):
    """_check of a float32 tensor [N, *shape_tail]."""
    _check(t, name, device, shape=None if shape_tail is None else ('N',) + tuple(shape_tail))


def check_density_state(rep, degree, best):
    """Range check of the state Engine.cluster_density_extend reads for its n_old old rows (tensors of [n_old] entries, any
    device): 0 <= rep[i] <= i, degree[i] >= 0, and every key best[i] is 0 or names a row < n_old (the row is 0xFFFFFFFF minus
    the key's low word).  Raises RuntimeError; plain torch, so it runs without a GPU."""
    n_old = rep.numel()
    if degree.numel() != n_old or best.numel() != n_old:
        raise RuntimeError('ffrnet_amd: density state of %d / %d / %d rows' % (n_old, degree.numel(), best.numel()))
    if n_old == 0:
        return
    rep, best = rep.reshape(-1).to(torch.int64), best.reshape(-1).to(torch.int64)
    row = torch.arange(n_old, device=rep.device, dtype=torch.int64)
    if bool(((rep < 0) | (rep > row)).any().item()):
        raise RuntimeError('ffrnet_amd: density state needs 0 <= rep[i] <= i (and so < %d)' % n_old)
    if bool((degree.reshape(-1) < 0).any().item()):
        raise RuntimeError('ffrnet_amd: density state needs degree >= 0')
    named = 0xFFFFFFFF - (best & 0xFFFFFFFF)
    if bool(((best != 0) & (named >= n_old)).any().item()):
        raise RuntimeError('ffrnet_amd: density state needs every key of best to be 0 or to name a row < %d' % n_old)


def tag_words(words, what, device=None):
    """The tag and mask words of the filtered search (include/ffrnet.h: ffr_search_topk_filtered) as the library reads them:
    a flat int32 tensor that carries the 32-bit patterns, on `device` when given.  Takes an int in [0, 2^32), an int32 tensor
    (its bits are the word: bit 31 shows as a negative value) or an int64 tensor with every value in [0, 2^32); anything else
    raises RuntimeError.  Plain torch, so it runs without a GPU."""
    if isinstance(words, bool) or not isinstance(words, (int, torch.Tensor)):
        raise RuntimeError('ffrnet_amd: %s must be an int or an int32 / int64 tensor, got %s' % (what, type(words)))
    if isinstance(words, int):
        if not 0 <= words < 2 ** 32:
            raise RuntimeError('ffrnet_amd: %s must lie in [0, 2^32), got %d' % (what, words))
        words = torch.tensor([words], dtype=torch.int64)
    if words.dtype not in (torch.int32, torch.int64):
        raise RuntimeError('ffrnet_amd: %s must be int32, or int64 in [0, 2^32), got %s' % (what, words.dtype))
    words = words.reshape(-1)
    if device is not None:
        words = words.to(device)
    if words.dtype == torch.int64:
        if words.numel() and (int(words.min().item()) < 0 or int(words.max().item()) >= 2 ** 32):
            raise RuntimeError('ffrnet_amd: %s: int64 words must lie in [0, 2^32)' % what)
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return words.contiguous()


_U8_HINT = ' (HWC, RGB)'


def _loss_weights(loss_weight):
    return (C.c_double * 4)(*[float(x) for x in loss_weight])


def _arith_code(arith):
    if arith not in ARITH:
        raise ValueError("ffrnet_amd: arith must be 'direct' or 'winograd', got %r" % (arith,))
    return ARITH[arith]


class Engine(object):
    """One native handle on one ROCm device: packed weights + workspace arena."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.device = torch.device('cuda', device if isinstance(device, int) else
                                   (device.index or 0))
        self._h = C.c_void_p(0)
        self._ck(self.lib.ffr_create(C.byref(self._h), self.device.index), create=True)
        self.has_encoder = False
        self.has_recnet = False
        self._recnet_sig = None      # lfw.pair_embed: signature of the RecNet shell whose weights this handle holds

    # -- plumbing -------------------------------------------------------------
    def _ck(self, rc, create=False):
        if rc != 0:
            msg = self.lib.ffr_last_error(None if create else self._h)
            raise RuntimeError('ffrnet native error %d: %s' % (rc, (msg or b'?').decode()))

    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            self.lib.ffr_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, fn, *args, stream=True):
        """One native call on this handle under its device context: fn(handle, *args[, torch's current stream]), status
        checked."""
        with torch.cuda.device(self.device):
            self._ck(fn(self._h, *args, self._stream()) if stream else fn(self._h, *args))

    def _tensor(self, t, name, dtype=torch.float32, shape=None, hint=''):
        """_check against this Engine's device: every tensor check of the class goes through here."""
        _check(t, name, self.device, dtype, shape, hint)

    def _flags(self, flip, n, name='flip'):
        """uint8 [n] device copy of per-image / per-pair flip flags (bool or uint8; nonzero = mirror), or None."""
        if flip is None:
            return None
        if not isinstance(flip, torch.Tensor) or flip.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError('ffrnet_amd: %s must be a bool or uint8 tensor, got %s'
                               % (name, flip.dtype if isinstance(flip, torch.Tensor) else type(flip)))
        if flip.numel() != n:
            raise RuntimeError('ffrnet_amd: %s must hold %d flags, got %d' % (name, n, flip.numel()))
        if flip.is_cuda and flip.device.index != self.device.index:
            raise RuntimeError('ffrnet_amd: %s is on %s but this Engine lives on %s' % (name, flip.device, self.device))
        return flip.reshape(-1).to(self.device, torch.uint8).contiguous()

    def _empty(self, *shape, dtype=torch.float32):
        return torch.empty(shape, device=self.device, dtype=dtype)

    def _embed_outputs(self, n, want_f, out=None):
        """(f_new[n,512], f[n,512] or None): new tensors, or the caller's preallocated pair `out` after its checks."""
        if out is None:
            return self._empty(n, 512), self._empty(n, 512) if want_f else None
        for o, nm in zip(out, ('out[0]', 'out[1]')):
            if o is not None:
                self._tensor(o, nm)
                if tuple(o.shape) != (n, 512) or not o.is_contiguous():
                    raise RuntimeError('ffrnet_amd: %s must be a contiguous [%d,512] tensor, got %s' % (nm, n, list(o.shape)))
        return out

    @staticmethod
    def _descs(sd):
        keep, items = [], []
        for k, v in sd.items():
            if not torch.is_tensor(v) or not v.is_floating_point():
                continue
            t = v.detach().to('cpu', torch.float32).contiguous()
            if t.dim() < 1 or t.dim() > 4:
                continue
            keep.append(t)
            d = TensorDesc()
            d.name = k.encode()
            d.data = t.data_ptr()
            d.ndim = t.dim()
            for i, s in enumerate(t.shape):
                d.shape[i] = s
            items.append(d)
        arr = (TensorDesc * len(items))(*items)
        return arr, len(items), keep

    # -- weights --------------------------------------------------------------
    def load_encoder(self, state_dict):
        arr, n, keep = self._descs(state_dict)
        self._ck(self.lib.ffr_load_encoder(self._h, arr, n))
        self.has_encoder = True
        nblk = 0
        while 'body.%d.res_layer.1.weight' % nblk in state_dict:
            nblk += 1
        self.num_layers = {24: 50, 49: 100, 50: 152}[nblk]

    def load_recnet(self, state_dict):
        arr, n, keep = self._descs(state_dict)
        self._ck(self.lib.ffr_load_recnet(self._h, arr, n))
        self.has_recnet = True
        self._recnet_sig = None      # whoever loaded through a shell records its signature after this call

    # -- forward --------------------------------------------------------------
    def _encoder_forward(self, fn, inputs, n, h, w, want_f, want_featmap):
        """encoder_forward and encoder_forward_u8 after their input checks"""
        if h % 16 or w % 16:
            raise RuntimeError('ffrnet_amd: H and W must be multiples of 16, got %dx%d' % (h, w))
        if want_f and (h, w) != (112, 112):
            # same failure as the reference: Linear(512*7*7, 512), model_ir_se50.py:124
            raise RuntimeError('mat1 and mat2 shapes cannot be multiplied (%dx%d and 25088x512)'
                               % (n, 512 * (h // 16) * (w // 16)))
        fm = self._empty(n, 512, h // 16, w // 16) if want_featmap else None
        f = self._empty(n, 512) if want_f else None
        self._call(fn, *[_ptr(t) for t in inputs], n, h, w, _ptr(fm), _ptr(f))
        return fm, f

    def encoder_forward(self, x, want_f=True, want_featmap=True):
        self._tensor(x, 'x')
        if x.dim() != 4 or x.size(1) != 3:
            raise RuntimeError('ffrnet_amd: encoder input must be [N,3,H,W], got %s' % list(x.shape))
        n, _, h, w = x.shape
        return self._encoder_forward(self.lib.ffr_encoder_forward, (x.contiguous(),), n, h, w, want_f, want_featmap)

    def encoder_forward_u8(self, img, flip=None, want_f=True, want_featmap=True):
        """encoder_forward from decoded images: img[N,H,W,3] uint8 HWC RGB (device), flip: optional bool / uint8 [N]
        per-image h-flip flags.  The input step (BGR swap, flip, ToTensor, Normalize(0.5, 0.5)) runs in the stem
        -> (featmap[N,512,H/16,W/16], f[N,512]), bit-identical to encoder_forward(O.preprocess_u8(img, flip))."""
        self._tensor(img, 'img', torch.uint8, ('N', 'H', 'W', 3), _U8_HINT)
        n, h, w, _ = img.shape
        return self._encoder_forward(self.lib.ffr_encoder_forward_u8, (img.contiguous(), self._flags(flip, n)), n, h, w,
                                     want_f, want_featmap)

    def recnet_forward(self, featmap, want_feat_new=True):
        self._tensor(featmap, 'input')
        if featmap.dim() != 4 or tuple(featmap.shape[1:]) != (512, 7, 7):
            c = featmap.size(1) + featmap.size(2) * featmap.size(3) if featmap.dim() == 4 else -1
            # the reference fails in Conv4Space's first conv (models/recnet.py:363)
            raise RuntimeError('RecNet expects input [N,512,7,7] (561 channels after the '
                               'self-similarity concat), got %s (%d channels)'
                               % (list(featmap.shape), c))
        featmap = featmap.contiguous()
        n = featmap.size(0)
        f_new = self._empty(n, 512)
        feat_new = self._empty(n, 512, 7, 7) if want_feat_new else None
        self._call(self.lib.ffr_recnet_forward, _ptr(featmap), n, _ptr(f_new), _ptr(feat_new))
        return f_new, feat_new

    def embed(self, x, want_f=True, out=None):
        """x[N,3,112,112] -> (f_new[N,512], f[N,512]); `out` = preallocated (f_new, f)."""
        self._tensor(x, 'x', shape=('N', 3, 112, 112))
        x = x.contiguous()
        n = x.size(0)
        f_new, f = self._embed_outputs(n, want_f, out)
        self._call(self.lib.ffr_embed, _ptr(x), n, _ptr(f_new), _ptr(f))
        return f_new, f

    def embed_u8(self, img, flip=None, want_f=True):
        """img[N,112,112,3] uint8 RGB (device) -> (f_new, f); flip: optional bool / uint8 [N] h-flip flags."""
        self._tensor(img, 'img', torch.uint8, ('N', 112, 112, 3), _U8_HINT)
        img = img.contiguous()
        n = img.size(0)
        fl = self._flags(flip, n)
        f_new, f = self._embed_outputs(n, want_f)
        self._call(self.lib.ffr_embed_u8, _ptr(img), _ptr(fl), n, _ptr(f_new), _ptr(f))
        return f_new, f

    def cosine_scores(self, a, b):
        self._tensor(a, 'a')
        self._tensor(b, 'b')
        if a.shape != b.shape or a.dim() != 2:
            raise RuntimeError('cosine_scores: a and b must both be [n,dim]')
        a, b = a.contiguous(), b.contiguous()
        s = self._empty(a.size(0))
        self._call(self.lib.ffr_cosine_scores, _ptr(a), _ptr(b), a.size(0), a.size(1), _ptr(s))
        return s

    def lfw_fold_accuracy(self, scores, labels, n_folds=10):
        """Device fold protocol: scores[n] fp32, labels[n] -> (mean accuracy, [(best_thr, acc)] per fold).
        The mean divides by n_folds (the reference hard-codes 10 = its n_folds)."""
        self._tensor(scores, 'scores')
        scores = scores.contiguous()
        if not torch.is_tensor(labels) or labels.numel() != scores.numel():      # the native call takes one n for both
            raise RuntimeError('ffrnet_amd: lfw_fold_accuracy needs one label per score: %d scores, %s labels'
                               % (scores.numel(), labels.numel() if torch.is_tensor(labels) else type(labels)))
        lab = labels.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        thr, acc = self._empty(n_folds, dtype=torch.float64), self._empty(n_folds, dtype=torch.float64)
        self._call(self.lib.ffr_lfw_fold_accuracy, _ptr(scores), _ptr(lab), scores.numel(), n_folds, _ptr(thr), _ptr(acc))
        thr, acc = thr.cpu().tolist(), acc.cpu().tolist()
        return sum(acc) / n_folds, list(zip(thr, acc))

    # -- 1:N identification (include/ffrnet.h: ffr_row_norms, ffr_search_topk, ffr_topk_merge) -------------------------
    def row_norms(self, x):
        """|x[r]| of x[n,512] rows (device fp32), the norms the search divides by -> norms[n]."""
        self._tensor(x, 'x')
        if x.dim() != 2:
            raise RuntimeError('ffrnet_amd: row_norms expects [n,dim], got %s' % list(x.shape))
        x = x.contiguous()
        out = self._empty(x.size(0))
        if x.size(0):
            self._call(self.lib.ffr_row_norms, _ptr(x), x.size(0), x.size(1), _ptr(out))
        return out

    def _search_inputs(self, query, gallery, gallery_norms, who):
        """The checks every search shares -> (query, gallery, gallery_norms, G), contiguous; the norms computed when not given"""
        self._tensor(query, 'query')
        self._tensor(gallery, 'gallery')
        if query.dim() != 2 or gallery.dim() != 2 or query.size(1) != gallery.size(1):
            raise RuntimeError('ffrnet_amd: %s expects query [Q,dim] and gallery [G,dim], got %s and %s'
                               % (who, list(query.shape), list(gallery.shape)))
        query, gallery = query.contiguous(), gallery.contiguous()
        G = gallery.size(0)
        if gallery_norms is None:
            gallery_norms = self.row_norms(gallery) if G else None
        else:
            self._tensor(gallery_norms, 'gallery_norms')
            if tuple(gallery_norms.shape) != (G,):
                raise RuntimeError('ffrnet_amd: gallery_norms must be [%d], got %s' % (G, list(gallery_norms.shape)))
            gallery_norms = gallery_norms.contiguous()
        return query, gallery, gallery_norms, G

    def _search(self, who, query, gallery, k, gallery_norms, index_base, coarse=None, subj=None, flt=None):
        """The body of the six searches.  coarse: (plane, flag) of search_coarse(); subj: (subjects, distinct) of
        search_subjects(); flt: (mask, tags) of search_filtered(), whose entry takes subjects or NULL in their place; coarse
        and flt together: search_coarse_filtered() -> [scores, index(, subjects)(, certified)].  The arguments go in the order of include/ffrnet.h; the tensors stay
        referenced until the call is made."""
        query, gallery, gallery_norms, G = self._search_inputs(query, gallery, gallery_norms, who)
        Q, k = query.size(0), int(k)

        def rows(t):                             # the gallery side: null pointers at G = 0
            return t if G else None
        name = 'ffr_search_topk'
        head, tail = [query, Q, rows(gallery), gallery_norms], [G, query.size(1), k, int(index_base)]
        null_out = []
        out = [self._empty(Q, max(k, 0)), self._empty(Q, max(k, 0), dtype=torch.int64)]
        if coarse is not None:
            plane, flag = coarse
            self._tensor(plane, 'plane', torch.int16, shape=(G, gallery.size(1)))
            self._tensor(flag, 'flag', torch.int32, shape=(1,))
            head += [rows(plane.contiguous()), flag]
            name += '_coarse'
        if flt is not None:
            mask, tags = tag_words(flt[0], 'mask', self.device), tag_words(flt[1], 'tags', self.device)
            if isinstance(flt[0], int):
                mask = mask.expand(Q).contiguous()
            if mask.numel() != Q or tags.numel() != G:
                raise RuntimeError('ffrnet_amd: %s expects mask [%d] (or an int) and tags [%d], got %d and %d words'
                                   % (who, Q, G, mask.numel(), tags.numel()))
            head.insert(1, mask)
            head.append(rows(tags))
            name += '_filtered'
            if subj is None:                     # NULL for gallery_subject and top_subject, distinct = 0
                head.append(None)
                tail.append(0)
                null_out = [None]
        if subj is not None:
            head.append(rows(self._subjects(subj[0], 'subjects', (G,))))
            tail.append(int(bool(subj[1])))
            out.append(self._empty(Q, max(k, 0), dtype=torch.int32))
            name += '_subjects' if flt is None else ''
        cert = [self._empty(Q, dtype=torch.int32)] if coarse is not None else []     # behind top_subject, NULL or not
        self._call(getattr(self.lib, name), *[a if isinstance(a, int) else _ptr(a) for a in head + tail + out + null_out + cert])
        return out + cert

    def search(self, query, gallery, k, gallery_norms=None, index_base=0):
        """Exact cosine top-k: query[Q,512], gallery[G,512] (device fp32) -> (scores[Q,k] fp32, index[Q,k] int64), per
        probe by descending score, ties by ascending index; index = index_base + gallery row; (-inf, -1) pads G < k.
        gallery_norms[G]: row_norms(gallery), computed here when not given (pass them when the gallery is reused)."""
        return tuple(self._search('search', query, gallery, k, gallery_norms, index_base))

    def coarse_pack(self, rows, norms, plane_out, flag):
        """plane_out[n,512] (int16: bf16 bits) = bf16(rows[r] / norms[r]) of rows[n,512]; flag (int32 [1], zero when its
        gallery was created) gets 1 ORed in when a row's norm is unsafe (include/ffrnet.h: ffr_coarse_pack)."""
        self._tensor(rows, 'rows', shape=('n', 512))
        n = rows.size(0)
        self._tensor(norms, 'norms', shape=(n,))
        self._tensor(plane_out, 'plane_out', torch.int16, shape=(n, 512))
        self._tensor(flag, 'flag', torch.int32, shape=(1,))
        if not (rows.is_contiguous() and norms.is_contiguous() and plane_out.is_contiguous()):
            raise RuntimeError('ffrnet_amd: coarse_pack expects contiguous rows, norms and plane_out')
        if n:
            self._call(self.lib.ffr_coarse_pack, _ptr(rows), _ptr(norms), n, 512, _ptr(plane_out), _ptr(flag))
        return plane_out

    def search_coarse(self, query, gallery, plane, flag, k, gallery_norms=None, index_base=0, return_certified=False):
        """search() through the certified bf16 shortlist (include/ffrnet.h: ffr_search_topk_coarse): the same
        (scores[Q,k], index[Q,k]) bit for bit.  plane[G,512] int16 and flag int32 [1] come from coarse_pack over the same
        rows and norms.  return_certified: also certified[Q] int32, 1 where the shortlist was proven to hold the top-k,
        0 where the probe went through the exact search."""
        out = self._search('search_coarse', query, gallery, k, gallery_norms, index_base, coarse=(plane, flag))
        return tuple(out if return_certified else out[:-1])

    def _topk_merge(self, who, scores, index, subj=None):
        """The body of the two merges.  subj: (subjects, distinct) of topk_merge_subjects() -> [scores, index(, subjects)]"""
        self._tensor(scores, 'scores')
        self._tensor(index, 'index', torch.int64)
        if scores.dim() != 3 or tuple(index.shape) != tuple(scores.shape):
            raise RuntimeError('ffrnet_amd: %s expects %s [S,Q,k], got %s and %s'
                               % (who, 'scores and index' if subj is None else 'scores, index and subjects',
                                  list(scores.shape), list(index.shape)))
        S, Q, k = scores.shape
        name = 'ffr_topk_merge'
        lists, dims = [scores.contiguous(), index.contiguous()], [S, Q, k]
        out = [self._empty(Q, k), self._empty(Q, k, dtype=torch.int64)]
        if subj is not None:
            lists.append(self._subjects(subj[0], 'subjects', (S, Q, k)))
            dims.append(int(bool(subj[1])))
            out.append(self._empty(Q, k, dtype=torch.int32))
            name += '_subjects'
        self._call(getattr(self.lib, name), *[_ptr(t) for t in lists], *dims, *[_ptr(t) for t in out])
        return out

    def topk_merge(self, scores, index):
        """Merge S sorted lists per probe, scores[S,Q,k] fp32 and index[S,Q,k] int64 (device; index < 0 = padding), in
        the order of search() -> (scores[Q,k], index[Q,k])."""
        return tuple(self._topk_merge('topk_merge', scores, index))

    # -- subject-labelled search (include/ffrnet.h: ffr_search_topk_subjects, ffr_topk_merge_subjects) -----------------
    def _subjects(self, t, name, shape):
        """int32 contiguous view or copy of subject ids (int32 or int64 on this Engine's device) of `shape`."""
        if isinstance(t, torch.Tensor) and t.dtype == torch.int64:
            self._tensor(t, name, torch.int64, shape)
            return t.to(torch.int32).contiguous()
        self._tensor(t, name, torch.int32, shape)
        return t.contiguous()

    def search_subjects(self, query, gallery, subjects, k, gallery_norms=None, index_base=0, distinct=True):
        """search() over a gallery whose rows carry a subject id: subjects[G] int32 or int64, >= 0 = the row's subject,
        < 0 = a removed row, which is never returned.  distinct=True (k <= 64): the top-k SUBJECTS, each once, by its best
        row (maximum score, then smallest index); distinct=False (k <= 128): the top-k live rows
        -> (scores[Q,k] fp32, index[Q,k] int64, subjects[Q,k] int32); (-inf, -1, -1) pads."""
        return tuple(self._search('search_subjects', query, gallery, k, gallery_norms, index_base, subj=(subjects, distinct)))

    def search_filtered(self, query, mask, gallery, tags, k, gallery_norms=None, index_base=0, subjects=None, distinct=False):
        """search() under a per-probe filter, one call for probes that may each see another part of the gallery
        (include/ffrnet.h: ffr_search_topk_filtered).  tags[G] is one 32-bit word per row, mask one per probe ([Q], or an int
        for all of them): row g is admissible for probe q iff tags[g] & mask[q] != 0.  Words are int32 tensors carrying the
        bit pattern, or int64 in [0, 2^32) (native.tag_words converts).  -> (scores[Q,k], index[Q,k]): search() over each
        probe's admissible rows, with their original indices; (-inf, -1) pads.  subjects[G] (as search_subjects() takes
        them): also removed rows are inadmissible, distinct as there (True: k <= 64), and the result is
        (scores, index, subjects[Q,k]), bit for bit search_subjects() over the gallery in which the rows inadmissible for
        the probe are marked removed."""
        if subjects is None and distinct:
            raise RuntimeError('ffrnet_amd: search_filtered: distinct=True needs subjects')
        return tuple(self._search('search_filtered', query, gallery, k, gallery_norms, index_base, flt=(mask, tags),
                                  subj=None if subjects is None else (subjects, distinct)))

    def search_coarse_subjects(self, query, gallery, plane, flag, subjects, k, gallery_norms=None, index_base=0, distinct=True,
                               return_certified=False):
        """search_subjects() through the certified bf16 shortlist (include/ffrnet.h: ffr_search_topk_coarse_subjects): the
        same (scores[Q,k], index[Q,k], subjects[Q,k]) bit for bit, in both modes and under every removal pattern.  plane and
        flag as search_coarse() takes them, subjects[G] as search_subjects() does.  The pass serves k <= 32 identities
        (distinct=True) and k <= 64 rows; above, the exact search runs alone.  return_certified: also certified[Q] int32."""
        out = self._search('search_coarse_subjects', query, gallery, k, gallery_norms, index_base, coarse=(plane, flag),
                           subj=(subjects, distinct))
        return tuple(out if return_certified else out[:-1])

    def search_coarse_filtered(self, query, mask, gallery, plane, flag, tags, k, gallery_norms=None, index_base=0, subjects=None,
                               distinct=False, return_certified=False):
        """search_filtered() through the certified bf16 shortlist (include/ffrnet.h: ffr_search_topk_coarse_filtered): the
        same tuples bit for bit, (scores, index) or with subjects (scores, index, subjects), for every tag and mask pattern.
        mask, tags, subjects and distinct as search_filtered() takes them, plane and flag as search_coarse() does.  The pass
        serves k <= 32 identities (distinct=True) and k <= 64 rows; above, the exact filtered search runs alone.
        return_certified: also certified[Q] int32, 1 where the shortlist of the probe's admissible rows was proven to hold
        its top-k (a probe with mask 0 is certified: all padding), 0 where the probe went through the exact search."""
        if subjects is None and distinct:
            raise RuntimeError('ffrnet_amd: search_coarse_filtered: distinct=True needs subjects')
        out = self._search('search_coarse_filtered', query, gallery, k, gallery_norms, index_base, coarse=(plane, flag),
                           flt=(mask, tags), subj=None if subjects is None else (subjects, distinct))
        return tuple(out if return_certified else out[:-1])

    def topk_merge_subjects(self, scores, index, subjects, distinct=True):
        """topk_merge() of lists that carry subjects: scores[S,Q,k] fp32, index[S,Q,k] int64, subjects[S,Q,k] int32 or
        int64; distinct=True keeps the first entry of every subject -> (scores[Q,k], index[Q,k], subjects[Q,k])."""
        return tuple(self._topk_merge('topk_merge_subjects', scores, index, subj=(subjects, distinct)))

    # -- clustering (include/ffrnet.h: ffr_cluster_threshold, ffr_cluster_templates) -----------------------------------
    def _cluster_rows(self, emb, norms, who):
        self._tensor(emb, 'emb')
        if emb.dim() != 2:
            raise RuntimeError('ffrnet_amd: %s expects emb [N,dim], got %s' % (who, list(emb.shape)))
        emb = emb.contiguous()
        if norms is not None:
            self._tensor(norms, 'norms')
            if tuple(norms.shape) != (emb.size(0),):
                raise RuntimeError('ffrnet_amd: norms must be [%d], got %s' % (emb.size(0), list(norms.shape)))
            norms = norms.contiguous()
        return emb, norms

    def _index_tensor(self, t, name):
        self._tensor(t, name, torch.int64, ('N',))
        return t.contiguous()

    def _out_rep(self, out, N):
        """the result tensor of a labelling: a new one, or the caller's `out` where that is a contiguous [N] int64 tensor"""
        if out is None:
            return self._empty(N, dtype=torch.int64)
        rep = self._index_tensor(out, 'out')
        if rep.numel() != N or rep.data_ptr() != out.data_ptr():
            raise RuntimeError('ffrnet_amd: out must be a contiguous [%d] int64 tensor' % N)
        return rep

    def _min_rows(self, min_rows, who):
        if int(min_rows) != min_rows or min_rows < 1:
            raise RuntimeError('ffrnet_amd: %s needs an integer min_rows >= 1, got %r' % (who, min_rows))

    def _n_old(self, n_old, N, who):
        if n_old < 0 or n_old > N:
            raise RuntimeError('ffrnet_amd: %s needs 0 <= n_old <= %d, got %d' % (who, N, n_old))

    def _keep_mask(self, keep, N):
        """keep[N], device bool or uint8 -> contiguous"""
        if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError('ffrnet_amd: keep must be a bool or uint8 tensor')
        self._tensor(keep, 'keep', keep.dtype, (N,))
        return keep.contiguous()

    def cluster(self, emb, threshold, norms=None):
        """Single-link clustering of emb[N,512] (device fp32) at one cosine threshold: rows i < j are joined iff their
        search score is > threshold -> rep[N] int64, rep[i] = the smallest row index of i's cluster.  norms[N]:
        row_norms(emb), computed in the call when not given."""
        emb, norms = self._cluster_rows(emb, norms, 'cluster')
        N = emb.size(0)
        rep = self._empty(N, dtype=torch.int64)
        self._call(self.lib.ffr_cluster_threshold, _ptr(emb if N else None), _ptr(norms), N, emb.size(1), float(threshold),
                   _ptr(rep))
        return rep

    def cluster_extend(self, emb, threshold, prior, n_old, norms=None, validate=True, out=None):
        """Extend a clustering by new rows: emb[N,512] holds all rows, the first n_old of them clustered before.  prior[N]
        (device int64) is a labelling in representative form, prior[i] <= i: the earlier rep for the old rows; for a new
        row the row itself, or an earlier row it is known to belong with.  Only the pairs i < j with j >= n_old are scored
        -> rep[N] int64, the smallest row of each component of (links i - prior[i]) + (scored edges): with prior[:n_old] =
        cluster(emb[:n_old]) and prior[j] = j for the new rows, exactly cluster(emb).  Pass flattened labels (prior[prior[i]]
        == prior[i]): deep chains are legal but walked hop by hop.  The kernel reads an entry outside [0, i] as i;
        `validate` range-checks prior here first (one small sync) and raises.  out: the result tensor, prior itself allowed."""
        emb, norms = self._cluster_rows(emb, norms, 'cluster_extend')
        prior = self._index_tensor(prior, 'prior')
        N, n_old = emb.size(0), int(n_old)
        if prior.numel() != N:
            raise RuntimeError('ffrnet_amd: prior must be [%d], got %s' % (N, list(prior.shape)))
        self._n_old(n_old, N, 'cluster_extend')
        if validate and N:
            row = torch.arange(N, device=prior.device, dtype=torch.int64)
            if bool(((prior < 0) | (prior > row)).any().item()):
                raise RuntimeError('ffrnet_amd: cluster_extend needs 0 <= prior[i] <= i (and so < %d)' % N)
        rep = self._out_rep(out, N)
        self._call(self.lib.ffr_cluster_extend, _ptr(emb if N else None), _ptr(norms), n_old, N, emb.size(1),
                   float(threshold), _ptr(prior if N else None), _ptr(rep if N else None))
        return rep

    def cluster_remove(self, emb, threshold, rep, keep, prior=None, norms=None, validate=True, out=None):
        """Take rows out of a single-link clustering: emb[N,512] holds all rows, rep[N] (device int64) their labels from
        cluster() or cluster_extend() at this threshold, keep[N] (device bool or uint8) is nonzero for the rows that stay.
        Nothing is moved -> rep[N] int64 in the same numbering: -1 for a removed row; the old label for every row of a
        cluster that lost no row; for the survivors of the clusters that lost one, the smallest row of their component when
        only they are joined again -- the labels of cluster() over the surviving rows, once compacted.  Only the pairs of
        those survivors are scored.  A label may rise (the representative was removed, or the cluster split).  prior[N]
        (device int64): must-links, prior[i] <= i the first SURVIVING row of i's tie group.  The kernels read an entry of rep
        or prior outside [0, i] as i; `validate` range-checks both here first (one small sync) and raises.  out: the result
        tensor, rep itself allowed.  Single link only: a density-gated clustering has cluster_density_remove."""
        emb, norms = self._cluster_rows(emb, norms, 'cluster_remove')
        rep_in = self._index_tensor(rep, 'rep')
        N = emb.size(0)
        if rep_in.numel() != N:
            raise RuntimeError('ffrnet_amd: rep must be [%d], got %s' % (N, list(rep_in.shape)))
        keep = self._keep_mask(keep, N)
        if prior is not None:
            prior = self._index_tensor(prior, 'prior')
            if prior.numel() != N:
                raise RuntimeError('ffrnet_amd: prior must be [%d], got %s' % (N, list(prior.shape)))
        if validate and N:
            row = torch.arange(N, device=rep_in.device, dtype=torch.int64)
            bad = (rep_in < 0) | (rep_in > row)
            if prior is not None:
                bad |= (prior < 0) | (prior > row)
            if bool(bad.any().item()):
                raise RuntimeError('ffrnet_amd: cluster_remove needs 0 <= rep[i] <= i and 0 <= prior[i] <= i (and so < %d)' % N)
        res = self._out_rep(out, N)
        self._call(self.lib.ffr_cluster_remove, _ptr(emb if N else None), _ptr(norms), N, emb.size(1), float(threshold),
                   _ptr(rep_in if N else None), _ptr(prior if N else None), _ptr(keep if N else None), _ptr(res if N else None))
        return res

    def cluster_density(self, emb, threshold, min_rows, norms=None, return_degree=False):
        """Density-gated clustering of emb[N,512] (device fp32) over the edges of cluster(): degree[i] = the rows scoring
        > threshold with i; a row is core iff degree[i] + 1 >= min_rows; clusters are the components of the core-core edges;
        a non-core row joins the cluster of its best-scoring core neighbour (ties: the smallest row) or stays alone
        -> (rep[N] int64, the smallest row index of each row's cluster; kind[N] uint8: 2 core, 1 border, 0 noise), and
        degree[N] int32 as a third entry with return_degree.  min_rows 1 and 2 give the rep of cluster()."""
        emb, norms = self._cluster_rows(emb, norms, 'cluster_density')
        self._min_rows(min_rows, 'cluster_density')
        N = emb.size(0)
        rep, kind = self._empty(N, dtype=torch.int64), self._empty(N, dtype=torch.uint8)
        degree = self._empty(N, dtype=torch.int32) if return_degree else None
        self._call(self.lib.ffr_cluster_density, _ptr(emb if N else None), _ptr(norms), N, emb.size(1), float(threshold),
                   int(min_rows), _ptr(rep if N else None), _ptr(kind if N else None), _ptr(degree if N else None))
        return (rep, kind, degree) if return_degree else (rep, kind)

    def cluster_density_extend(self, emb, threshold, min_rows, rep, degree, best, n_old, norms=None, validate=True):
        """Extend a density-gated clustering by new rows: emb[N,512] holds all rows, the first n_old of them clustered
        before at this threshold and min_rows.  The state of those rows is rep (int64), degree (int32) and best (int64: the
        64 bits of the key by which a border row chose its core row, 0 for core and noise rows), each [n_old] or [N]; a
        tensor of [N] entries is updated in place, and with n_old = 0 each may be None.  -> (rep, kind, degree, best), all
        [N]: rep, kind and degree equal cluster_density(emb, ..., return_degree=True) when the state is the one an earlier
        call left for emb[:n_old], and best is the state for the next call.  n_old = 0 clusters from scratch.  The kernels
        read out-of-range state as "none"; `validate` range-checks it here first (check_density_state, one small sync)."""
        emb, norms = self._cluster_rows(emb, norms, 'cluster_density_extend')
        self._min_rows(min_rows, 'cluster_density_extend')
        N, n_old = emb.size(0), int(n_old)
        self._n_old(n_old, N, 'cluster_density_extend')
        state = []
        for t, name, dtype in ((rep, 'rep', torch.int64), (degree, 'degree', torch.int32), (best, 'best', torch.int64)):
            if t is None and n_old == 0:
                t = self._empty(N, dtype=dtype)
            self._tensor(t, name, dtype, ('N',))
            if t.numel() not in (n_old, N):
                raise RuntimeError('ffrnet_amd: %s must be [%d] or [%d], got %s' % (name, n_old, N, list(t.shape)))
            if t.numel() != N or not t.is_contiguous():
                full = self._empty(N, dtype=dtype)
                full[:n_old] = t[:n_old]
                t = full
            state.append(t)
        rep, degree, best = state
        if validate:
            check_density_state(rep[:n_old], degree[:n_old], best[:n_old])
        kind = self._empty(N, dtype=torch.uint8)
        self._call(self.lib.ffr_cluster_density_extend, _ptr(emb if N else None), _ptr(norms), n_old, N, emb.size(1),
                   float(threshold), int(min_rows), _ptr(rep if N else None), _ptr(kind if N else None),
                   _ptr(degree if N else None), _ptr(best if N else None))
        return rep, kind, degree, best

    def cluster_density_remove(self, emb, threshold, min_rows, rep, degree, best, keep, norms=None, validate=True):
        """Take rows out of a density-gated clustering: emb[N,512] holds all rows; rep (int64), degree (int32) and best
        (int64), each [N], are the state cluster_density_extend left for them at this threshold and min_rows; keep[N] (device
        bool or uint8) is nonzero for the rows that stay.  Nothing is moved -> (rep, kind, degree, best), all [N], in the same
        numbering; contiguous state tensors are updated in place.  On the surviving rows the result is, once compacted,
        cluster_density(emb[keep], ..., return_degree=True), and best (its core rows renumbered) the state of
        cluster_density_extend over emb[keep] from scratch; a removed row gets -1 / 0 / 0 / 0.  A label may rise and a border
        row may change its cluster.  Scored are the removed rows against all rows, the pairs among the still-core rows of the
        clusters that lost a core row, and the rows that have to choose a core row again against all rows.  The kernels read
        out-of-range state as "none"; `validate` range-checks it here first (check_density_state, one small sync)."""
        emb, norms = self._cluster_rows(emb, norms, 'cluster_density_remove')
        self._min_rows(min_rows, 'cluster_density_remove')
        N = emb.size(0)
        state = []
        for t, name, dtype in ((rep, 'rep', torch.int64), (degree, 'degree', torch.int32), (best, 'best', torch.int64)):
            self._tensor(t, name, dtype, ('N',))
            if t.numel() != N:
                raise RuntimeError('ffrnet_amd: %s must be [%d], got %s' % (name, N, list(t.shape)))
            state.append(t.contiguous())
        rep, degree, best = state
        keep = self._keep_mask(keep, N)
        if validate:
            check_density_state(rep, degree, best)
        kind = self._empty(N, dtype=torch.uint8)
        self._call(self.lib.ffr_cluster_density_remove, _ptr(emb if N else None), _ptr(norms), N, emb.size(1), float(threshold),
                   int(min_rows), _ptr(keep if N else None), _ptr(rep if N else None), _ptr(kind if N else None),
                   _ptr(degree if N else None), _ptr(best if N else None))
        return rep, kind, degree, best

    def cluster_templates(self, emb, order, offsets, norms=None, validate=True):
        """One template per cluster: order (int64, rows of emb sorted by cluster then index) and offsets[C+1] (int64,
        ascending) -> templates[C,512], row c = the normalised sum of the normalised rows order[offsets[c]:offsets[c+1]].
        The kernel trusts both; `validate` range-checks them here first (one small sync)."""
        emb, norms = self._cluster_rows(emb, norms, 'cluster_templates')
        order, offsets = self._index_tensor(order, 'order'), self._index_tensor(offsets, 'offsets')
        if offsets.numel() < 1:
            raise RuntimeError('ffrnet_amd: offsets must hold C + 1 entries')
        Cn = offsets.numel() - 1
        if validate and Cn:
            d = offsets[1:] - offsets[:-1]
            bad = bool(((offsets[0] < 0) | (d.min() < 0) | (offsets[-1] > order.numel())).item())
            if not bad and order.numel():
                bad = bool(((order.min() < 0) | (order.max() >= emb.size(0))).item())
            if bad:
                raise RuntimeError('ffrnet_amd: cluster_templates needs 0 <= order < %d and ascending offsets within '
                                   '[0, %d]' % (emb.size(0), order.numel()))
        out = self._empty(Cn, emb.size(1))
        self._call(self.lib.ffr_cluster_templates, _ptr(emb if emb.size(0) else None), _ptr(norms), _ptr(order),
                   _ptr(offsets), Cn, emb.size(1), _ptr(out))
        return out

    # -- face alignment (include/ffrnet.h: ffr_align_transforms, ffr_align_warp, ffr_embed_aligned) -------------------
    def _align_points(self, landmarks, template):
        """device copies of landmarks [N,K,2] and the template [K,2] -> (landmarks, template, N, K)"""
        tmpl = _align.as_template(template)
        K = tmpl.size(0)
        N = _align.check_landmarks(landmarks, K)
        self._tensor(landmarks, 'landmarks')
        return landmarks.contiguous(), tmpl.to(self.device), N, K

    def _align_frames(self, frames, frame_index, N):
        """frames [F,H,W,3] uint8 (rows may be padded) and frame_index [N] -> (frames, pitch_bytes, int32 frame_index)"""
        self._tensor(frames, 'frames', torch.uint8, ('F', 'H', 'W', 3), _U8_HINT)
        if frames.size(0) < 1 or frames.size(1) < 1 or frames.size(2) < 1:
            raise RuntimeError('ffrnet_amd: frames must not be empty, got %s' % list(frames.shape))
        pitch = _align.frame_pitch(frames)
        if pitch is None:
            frames = frames.contiguous()
            pitch = 3 * frames.size(2)
        _align.check_frame_bytes(pitch, frames.size(1))
        if not isinstance(frame_index, torch.Tensor) or frame_index.dtype not in (torch.int32, torch.int64):
            raise RuntimeError('ffrnet_amd: frame_index must be an int32 or int64 tensor')
        if frame_index.numel() != N:
            raise RuntimeError('ffrnet_amd: frame_index must hold %d entries, got %d' % (N, frame_index.numel()))
        if frame_index.is_cuda and frame_index.device.index != self.device.index:
            raise RuntimeError('ffrnet_amd: frame_index is on %s but this Engine lives on %s' % (frame_index.device, self.device))
        return frames, pitch, frame_index.reshape(-1).to(self.device, torch.int32).contiguous()

    def align_transforms(self, landmarks, template=_align.TEMPLATE_112x112):
        """landmarks[N,K,2] fp32 (device; (x, y) in the face's frame) and the template's K points in the crop ->
        (A float64 [N,6], valid uint8 [N]): the row-major 2x3 similarity crop -> frame of the reference's cp2tform fit,
        valid = 0 (and A = 0) for degenerate or non-finite landmarks."""
        landmarks, tmpl, N, K = self._align_points(landmarks, template)
        A, valid = self._empty(N, 6, dtype=torch.float64), self._empty(N, dtype=torch.uint8)
        self._call(self.lib.ffr_align_transforms, _ptr(landmarks), _ptr(tmpl), N, K, _ptr(A), _ptr(valid))
        return A, valid

    def align_warp(self, frames, frame_index, A, valid=None, out_hw=(112, 112)):
        """frames[F,H,W,3] uint8 (device; rows may be padded: the pitch is its row stride), frame_index[N], A[N,6]
        float64 -> crops uint8 [N,h,w,3] by the exact 1/32-pixel bilinear rule of include/ffrnet.h; zeros where
        valid[n] == 0 or frame_index[n] is outside [0,F)."""
        oh, ow = _align.check_out_hw(out_hw)
        self._tensor(A, 'A', torch.float64, ('N', 6))
        N = A.size(0)
        if N < 1:
            raise RuntimeError('ffrnet_amd: A must be float64 [N,6] with N >= 1, got %s' % list(A.shape))
        frames, pitch, fidx = self._align_frames(frames, frame_index, N)
        v = self._flags(valid, N, 'valid')
        crop = self._empty(N, oh, ow, 3, dtype=torch.uint8)
        self._call(self.lib.ffr_align_warp, _ptr(frames), frames.size(0), frames.size(1), frames.size(2), pitch, _ptr(fidx),
                   _ptr(A.contiguous()), _ptr(v), N, oh, ow, _ptr(crop))
        return crop

    def align_crops(self, frames, frame_index, landmarks, template=_align.TEMPLATE_112x112, out_hw=(112, 112)):
        """align_transforms + align_warp -> crops uint8 [N,h,w,3] (zeros for a face that is not valid)."""
        A, valid = self.align_transforms(landmarks, template)
        return self.align_warp(frames, frame_index, A, valid, out_hw)

    def embed_aligned(self, frames, frame_index, landmarks, template=_align.TEMPLATE_112x112, flip=None, want_f=True):
        """Detector output to embeddings in one call: transforms, the 112x112 warp into the handle's scratch and the
        embed_u8 pipeline -> (f_new[N,512], f[N,512] or None, valid uint8 [N]); bit-identical to
        embed_u8(align_crops(...), flip).  valid[n] == 0 (degenerate landmarks, or a frame_index outside [0,F)): the row is
        the embedding of a zero crop, to be dropped."""
        landmarks, tmpl, N, K = self._align_points(landmarks, template)
        frames, pitch, fidx = self._align_frames(frames, frame_index, N)
        fl = self._flags(flip, N)
        f_new, f = self._embed_outputs(N, want_f)
        valid = self._empty(N, dtype=torch.uint8)
        self._call(self.lib.ffr_embed_aligned, _ptr(frames), frames.size(0), frames.size(1), frames.size(2), pitch, _ptr(fidx),
                   _ptr(landmarks), _ptr(tmpl), K, _ptr(fl), N, _ptr(f_new), _ptr(f), _ptr(valid))
        return f_new, f, valid

    # -- arena / measurement --------------------------------------------------
    def workspace_bytes(self, n, h=112, w=112):
        return int(self.lib.ffr_workspace_bytes(self._h, n, h, w))

    def reserve(self, n, h=112, w=112):
        self._call(self.lib.ffr_reserve, n, h, w, stream=False)

    def set_option(self, name, value):
        """Experiment knob of this handle (include/ffrnet.h: ffr_set_option); the library reads no environment."""
        self._call(self.lib.ffr_set_option, name.encode(), int(value), stream=False)

    def get_option(self, name):
        v = C.c_longlong(0)
        self._ck(self.lib.ffr_get_option(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def set_options_from_env(self, prefix='FFR_OPT_'):
        """tools/ only: FFR_OPT_<NAME>=<int> in the environment of a measurement script -> set_option(name, int).
        Read here, in the script's own host code; libffrnet_hip.so itself never looks at the environment."""
        done = {}
        for k, v in sorted(os.environ.items()):
            if k.startswith(prefix):
                self.set_option(k[len(prefix):].lower(), int(v))
                done[k[len(prefix):].lower()] = int(v)
        return done

    def generation(self):
        """Changes whenever the handle released device memory a captured hipGraph may point into."""
        return int(self.lib.ffr_generation(self._h))

    # -- per-layer arithmetic (include/ffrnet.h: ffr_layer_*, ffr_calibrate) ----------------------------
    def layers(self):
        """The Winograd-eligible convolutions of the loaded nets: [{index, name, net, arith, sensitivity}], name = the
        conv's state_dict prefix, net 'encoder' | 'recnet', arith 'direct' | 'winograd', sensitivity from the last
        calibrate() (None before)."""
        n = C.c_int(0)
        self._ck(self.lib.ffr_layer_count(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            li = LayerInfo()
            self._ck(self.lib.ffr_layer_get(self._h, i, C.byref(li)))
            out.append(dict(index=i, name=li.name.decode(), net=('encoder', 'recnet')[li.net],
                            arith='direct' if li.arith == 0 else 'winograd',
                            sensitivity=li.sensitivity if li.sensitivity >= 0 else None))
        return out

    def _layer_index(self, name_or_index):
        if isinstance(name_or_index, int):
            return name_or_index
        for l in self.layers():
            if l['name'] == name_or_index:
                return l['index']
        raise KeyError('ffrnet_amd: no Winograd-eligible layer named %r' % (name_or_index,))

    def set_layer_arith(self, name_or_index, arith):
        """Pin one layer to 'direct' or return it to 'winograd'.  Changes generation() (captured graphs re-capture)."""
        code = _arith_code(arith)
        self._ck(self.lib.ffr_layer_set_arith(self._h, self._layer_index(name_or_index), code))

    def arithmetic_plan(self, net=None):
        """{layer name: 'direct' | 'winograd'} of the loaded nets (or of one net: 'encoder' | 'recnet')."""
        return {l['name']: l['arith'] for l in self.layers() if net is None or l['net'] == net}

    def set_arithmetic_plan(self, plan, net=None):
        """Apply a {name: 'direct' | 'winograd'} mapping; the layers it does not name (of `net`, or of every loaded net)
        return to Winograd.  Unknown names raise KeyError."""
        known = {l['name']: l for l in self.layers()}
        for name, arith in plan.items():
            if name not in known:
                raise KeyError('ffrnet_amd: no Winograd-eligible layer named %r' % (name,))
            _arith_code(arith)
        for name, l in known.items():
            if net is None or l['net'] == net:
                want = plan.get(name, 'winograd')
                if want != l['arith']:
                    self._ck(self.lib.ffr_layer_set_arith(self._h, l['index'], ARITH[want]))

    def calibrate(self, x=None, featmap=None, tol=1e-4):
        """Pin layers to direct only as far as needed for this handle's forward on these inputs (x[N,3,H,W] images or
        featmap[N,512,7,7], exactly one) to stay within tol * abs-max of its all-direct forward, per output tensor
        (ffr_calibrate).  Synchronises.  -> {'tol', 'n', 'layers': [{name, net, sensitivity, arith}], 'achieved':
        {f, featmap, f_new, feat_new: value or None where the forward has no such output}}.  Calibrate at the batch size
        you will run: the Winograd kernels depend on it."""
        if (x is None) == (featmap is None):
            self._call(self.lib.ffr_calibrate, _ptr(x), _ptr(featmap), 1, 112, 112, float(tol), None)      # raises
        t = x if x is not None else featmap
        self._tensor(t, 'x' if x is not None else 'featmap')
        t = t.contiguous()
        if x is not None and (t.dim() != 4 or t.size(1) != 3):
            raise RuntimeError('ffrnet_amd: calibration images must be [N,3,H,W], got %s' % list(t.shape))
        if featmap is not None and (t.dim() != 4 or tuple(t.shape[1:]) != (512, 7, 7)):
            raise RuntimeError('ffrnet_amd: a calibration featmap must be [N,512,7,7], got %s' % list(t.shape))
        n, _, h, w = t.shape
        ach = (C.c_double * 4)()
        self._call(self.lib.ffr_calibrate, _ptr(x if x is None else t), _ptr(featmap if featmap is None else t), n, h, w,
                   float(tol), ach)
        return dict(tol=float(tol), n=int(n),
                    layers=[dict(name=l['name'], net=l['net'], sensitivity=l['sensitivity'], arith=l['arith']) for l in self.layers()],
                    achieved={k: (ach[i] if ach[i] >= 0 else None) for i, k in enumerate(CALIB_TENSORS)})

    def memory_stats(self):
        """Device bytes and packing seconds of the handle (include/ffrnet.h: ffr_mem_stats)."""
        st = MemStats()
        self._ck(self.lib.ffr_memory_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in MemStats._fields_}

    def probe_mfma_peak(self, iters=20000):
        """(TFLOP/s, shader clock in GHz) of a register-resident fp32-MFMA loop on this device."""
        tf, ghz = C.c_double(0), C.c_double(0)
        self._call(self.lib.ffr_probe_mfma_peak, iters, C.byref(tf), C.byref(ghz))
        return tf.value, ghz.value

    def profile_enable(self, on=True):
        self._ck(self.lib.ffr_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        arr = (KClassStat * len(KCLASS_NAMES))()
        self._ck(self.lib.ffr_profile_read(self._h, arr))
        return {KCLASS_NAMES[i]: dict(launches=int(arr[i].launches), ms=arr[i].ms,
                                      flops=arr[i].flops, bytes=arr[i].bytes, flops_executed=arr[i].flops_executed,
                                      flops_useful=arr[i].flops_useful)
                for i in range(len(KCLASS_NAMES))}

    # -- test hooks -----------------------------------------------------------
    def op_conv(self, **kw):
        d = ConvDesc()
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                v = v.data_ptr()
            elif v is None:
                v = 0 if k not in ('x', 'w', 'bias', 'slope', 'resid', 'out') else None
            setattr(d, k, v)
        self._call(self.lib.ffr_op_conv, C.byref(d))

    def op_conv3x3(self, x_nhwc, w, bias, slope=None, pad_mode=0, use_wino=True, resid=None):
        """x[N,H,W,cin] device NHWC, w[cout,cin,3,3] / bias / slope host tensors -> out[N,H,W,cout]."""
        self._tensor(x_nhwc, 'x')
        x_nhwc = x_nhwc.contiguous()
        n, hh, ww, cin = x_nhwc.shape
        wh = w.detach().float().cpu().contiguous()
        bh = bias.detach().float().cpu().contiguous()
        sh = slope.detach().float().cpu().contiguous() if slope is not None else None
        out = self._empty(n, hh, ww, wh.size(0))
        self._call(self.lib.ffr_op_conv3x3, _ptr(x_nhwc), n, hh, ww, cin, _ptr(wh), _ptr(bh), _ptr(sh), wh.size(0), pad_mode,
                   int(use_wino), _ptr(resid.contiguous() if resid is not None else None), _ptr(out))
        return out

    def op_conv3x3_ex(self, x, w, bias, out, cin=None, slope=None, in_scale=None, in_shift=None, resid=None, out_coff=0,
                      cout_store=0, pad_mode=0, use_wino=-1, sigmoid=False, tile_sums=None):
        """The 3x3 / stride 1 / pad 1 convolution with the whole epilogue contract (test hook).  x [N,H,W,in_pitch], out
        [N,H,W,out_pitch], resid [N,H,W,res_pitch] and tile_sums [T,cout_pad] are device tensors, written / read in place at
        their own pitches; w [cout,cin,3,3], bias, slope, in_scale, in_shift host tensors.  use_wino -1: the planner's choice."""
        for t, name in ((x, 'x'), (out, 'out')) + (((resid, 'resid'),) if resid is not None else ()) + \
                (((tile_sums, 'tile_sums'),) if tile_sums is not None else ()):
            self._tensor(t, name)
            if not t.is_contiguous():
                raise RuntimeError('ffrnet_amd: %s must be contiguous' % name)
        host = [None if t is None else t.detach().float().cpu().contiguous() for t in (w, bias, slope, in_scale, in_shift)]
        d = Conv3x3Desc()
        d.x = x.data_ptr(); d.N, d.H, d.W, d.in_pitch = x.shape
        d.cin = host[0].size(1) if cin is None else cin
        d.w_host, d.bias_host, d.slope_host, d.in_scale_host, d.in_shift_host = [None if t is None else t.data_ptr() for t in host]
        d.cout = host[0].size(0)
        d.resid = resid.data_ptr() if resid is not None else None
        d.res_pitch = resid.size(3) if resid is not None else 0
        d.out = out.data_ptr(); d.out_pitch = out.size(3); d.out_coff = out_coff; d.cout_store = cout_store
        d.pad_mode = pad_mode; d.use_wino = int(use_wino); d.flags = 1 if sigmoid else 0
        d.tile_sums = tile_sums.data_ptr() if tile_sums is not None else None
        self._call(self.lib.ffr_op_conv3x3_ex, C.byref(d))

    def conv_plan_record(self, on=True):
        """Switches the plan record of the convolution launchers on (clearing it) or off (test hook)."""
        self._ck(self.lib.ffr_conv_plan_record(self._h, 1 if on else 0))

    def conv_plan(self):
        """The convolution launches since conv_plan_record(True), in launch order: [{path ('direct' | 'fused' |
        'unfused-gemm-stream' | 'unfused-igemm' | 'mixed' | 'tail-split' | 'channel' = RecNet's k_channel_path), images, rows, tile, nblocks, granule, nkt, tiles, cut,
        split, phased, half_n, block_tiles, n_main, side, stride, conv_shortcut, se_scale}] (include/ffrnet.h: ffr_conv_launch).
        The encoder trunk adds its glue launches: 'se-pool' | 'se-tiles' (SE squeeze by its own pass | from tile sums: rows = H*W,
        tiles = S), 'combine' | 'combine-in-c' | 'combine-in-mixed' (one per bottleneck, its last entry: rows = H*W, tiles per
        image, stride, conv_shortcut, se_scale) and 'wino-out-in' (the chained conv1 -> conv2 transform: rows = T, tiles per image)."""
        n = C.c_int(0)
        self._ck(self.lib.ffr_conv_plan_read(self._h, None, 0, C.byref(n)))
        arr = (ConvLaunch * max(n.value, 1))()
        self._ck(self.lib.ffr_conv_plan_read(self._h, arr, n.value, C.byref(n)))
        out = []
        for i in range(n.value):
            d = {f: getattr(arr[i], f) for f, _ in ConvLaunch._fields_}
            d['path'] = CONV_PATHS[d['path']]
            out.append(d)
        return out

    def op_convlayer_train(self, x_nhwc, G, w, gamma, beta, slope, da_nhwc, need_dx=True):
        """One ConvLayer in train() mode (models/recnet.py:78-85), forward + backward (test hook).
        x_nhwc [G*N,7,7,cin] and da_nhwc [G*N,7,7,cout] device tensors (logical channel counts);
        w [cout,cin,3,3], gamma/beta/slope [cout] host tensors.
        Returns dict(out, dx, dw[cout,cin,3,3], dgamma, dbeta, dslope, running_mean, running_var, mean, invstd)."""
        self._tensor(x_nhwc, 'x')
        gn, hh, ww, cin = x_nhwc.shape
        assert hh == 7 and ww == 7 and gn % G == 0
        cout = w.size(0)
        cin_pad, cout_pad = (cin + 31) // 32 * 32, (cout + 63) // 64 * 64
        rows = gn * 49
        dev = x_nhwc.device
        xp = torch.zeros((rows, cin_pad), device=dev)
        xp[:, :cin] = x_nhwc.reshape(rows, cin)
        dap = torch.zeros((rows, cout_pad), device=dev)
        dap[:, :cout] = da_nhwc.reshape(rows, cout)
        host = [t.detach().float().cpu().contiguous() for t in (w, gamma, beta, slope)]
        out = torch.empty((rows, cout_pad), device=dev)
        dx = torch.zeros((rows, cin_pad), device=dev) if need_dx else None
        dw = torch.empty((cout_pad, 9, cin_pad), device=dev)
        dvec = torch.empty((5, cout_pad), device=dev)
        stats = torch.empty((2, G, cout_pad), device=dev)
        self._call(self.lib.ffr_op_convlayer_train, _ptr(xp), G, gn // G, cin, cout, *[_ptr(t) for t in host], _ptr(dap),
                   _ptr(out), _ptr(dx), _ptr(dw), _ptr(dvec), _ptr(stats))
        dwt = dw[:cout, :, :cin].reshape(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous()
        return dict(out=out[:, :cout].reshape(gn, 7, 7, cout), dx=dx[:, :cin].reshape(gn, 7, 7, cin) if need_dx else None,
                    dw=dwt, dgamma=dvec[0, :cout], dbeta=dvec[1, :cout], dslope=dvec[2, :cout],
                    running_mean=dvec[3, :cout], running_var=dvec[4, :cout], mean=stats[0, :, :cout],
                    invstd=stats[1, :, :cout])

    # -- RecNet training step (include/ffrnet_train.h) --------------------------------------------
    N_CLASSES = 10575
    _WHICH = {'param': 0, 'grad': 1, 'exp_avg': 2, 'exp_avg_sq': 3, 'running': 4}
    validate_labels = True     # range check of class ids (the reference fails loudly in scatter_ / CrossEntropyLoss)

    def _labels(self, label, n, device):
        """int32 device copy of `label` after the checks the native kernels do not make: one id per image, every id in
        [0, N_CLASSES).  A CPU tensor is checked before the copy (free); a device tensor costs one small sync, which
        `validate_labels = False` removes."""
        if not torch.is_tensor(label) or label.numel() != n:
            raise RuntimeError('ffrnet_amd: expected %d class labels, got %s' %
                               (n, list(label.shape) if torch.is_tensor(label) else type(label)))
        if self.validate_labels and n:
            lo, hi = int(label.min()), int(label.max())
            if lo < 0 or hi >= self.N_CLASSES:
                raise RuntimeError('ffrnet_amd: class label out of range [0, %d): min %d, max %d' % (self.N_CLASSES, lo, hi))
        return label.reshape(-1).to(device, torch.int32).contiguous()

    def train_init(self, recnet_state_dict):
        """Device-resident training state (flat parameter / gradient / Adam buffers) from a RecNet state_dict."""
        arr, n, keep = self._descs(recnet_state_dict)
        self._ck(self.lib.ffr_train_init(self._h, arr, n))
        self._train_spec = {k: tuple(v.shape) for k, v in recnet_state_dict.items()}
        # num_batches_tracked continues from the loaded values (the native counter counts updates since this call)
        self._nbt0 = {k: int(v) for k, v in recnet_state_dict.items() if k.endswith('num_batches_tracked')}

    def train_info(self):
        p, g, n, nbt, step = _P(0), _P(0), C.c_size_t(0), C.c_longlong(0), C.c_int(0)
        self._ck(self.lib.ffr_train_info(self._h, C.byref(p), C.byref(g), C.byref(n), C.byref(nbt), C.byref(step)))
        return dict(params=p.value, grads=g.value, n_flat=n.value, num_batches_tracked=nbt.value, adam_step=step.value)

    def train_get(self, key, which='param'):
        """One tensor in torch layout on the host; which: param | grad | exp_avg | exp_avg_sq | running."""
        out = torch.empty(self._train_spec[key], dtype=torch.float32)
        self._ck(self.lib.ffr_train_get(self._h, self._WHICH[which], key.encode(), C.c_void_p(out.data_ptr()), out.numel()))
        return out

    def train_set(self, key, value, which='param'):
        v = value.detach().to('cpu', torch.float32).contiguous()
        self._ck(self.lib.ffr_train_set(self._h, self._WHICH[which], key.encode(), C.c_void_p(v.data_ptr()), v.numel()))

    def train_state_dict(self):
        """The RecNet state_dict as the reference would save it (models/trainer.py:216-224)."""
        info = self.train_info()
        sd = {}
        for k, shape in self._train_spec.items():
            if k.endswith('num_batches_tracked'):
                sd[k] = torch.tensor(info['num_batches_tracked'] + self._nbt0.get(k, 0), dtype=torch.long)
            elif k.endswith(('running_mean', 'running_var')):
                sd[k] = self.train_get(k, 'running')
            else:
                sd[k] = self.train_get(k, 'param')
        return sd

    def train_zero_grad(self):
        self._call(self.lib.ffr_train_zero_grad)

    def train_forward(self, featmap, label, groups=1, slot=0, want=('f_new', 'pred_loss', 'pred_label', 'M_space',
                                                                      'M_channel', 'feat_space', 'feat_channel')):
        """RecNet.forward(input, label) in train() mode on `groups` BatchNorm batches stacked along dim 0.
        Returns the reference's 7-tuple (entries not in `want` are None)."""
        self._tensor(featmap, 'featmap')
        featmap = featmap.contiguous()
        n = featmap.size(0)
        if featmap.dim() != 4 or tuple(featmap.shape[1:]) != (512, 7, 7) or n % groups:
            raise RuntimeError('ffrnet_amd: RecNet input must be [G*N,512,7,7], got %s' % list(featmap.shape))
        lab = self._labels(label, n, featmap.device)
        shapes = dict(f_new=(n, 512), pred_loss=(n, self.N_CLASSES), pred_label=(n, self.N_CLASSES), M_space=(n, 49, 49),
                      M_channel=(n, 512, 512), feat_space=(n, 512, 7, 7), feat_channel=(n, 512, 7, 7))
        names = ('f_new', 'pred_loss', 'pred_label', 'M_space', 'M_channel', 'feat_space', 'feat_channel')
        outs = [self._empty(*shapes[k]) if k in want else None for k in names]
        self._call(self.lib.ffr_train_forward, slot, _ptr(featmap), _ptr(lab), groups, n // groups, *[_ptr(o) for o in outs])
        return tuple(outs)

    def train_backward(self, grads, slot=0):
        """grads: 7 tensors or None (gradients wrt the 7-tuple of train_forward); adds into the flat gradient buffer."""
        gs = [g.contiguous().float() if g is not None else None for g in grads]
        for g in gs:
            if g is not None:
                self._tensor(g, 'grad')
        self._call(self.lib.ffr_train_backward, slot, *[_ptr(g) for g in gs])

    def train_export(self, key, out, which='grad'):
        """One entry in torch layout into the device tensor `out` (no host round trip)."""
        self._tensor(out, 'out')
        assert out.is_contiguous()
        self._call(self.lib.ffr_train_export, self._WHICH[which], key.encode(), _ptr(out))
        return out

    def train_import(self, key, value, which='param'):
        self._tensor(value, 'value')
        v = value.detach().contiguous()
        self._call(self.lib.ffr_train_import, self._WHICH[which], key.encode(), _ptr(v))

    def train_losses(self, f_enc, loss_weight=(1, 1, 1, 1), slot=0):
        """The four weighted loss items + accuracy (device tensor [5]) of the forward in `slot` (G = 2)."""
        self._tensor(f_enc, 'f_enc')
        out = self._empty(5)
        self._call(self.lib.ffr_train_losses, slot, _ptr(f_enc.contiguous()), _loss_weights(loss_weight), _ptr(out))
        return out

    def train_backward_losses(self, slot=0):
        self._call(self.lib.ffr_train_backward_losses, slot)

    def train_iteration(self, img_non, img_ocl, label, loss_weight=(1, 1, 1, 1)):
        """Encoder + RecNet train forward + losses + zero_grad + backward in one native call -> device tensor [5]."""
        self._tensor(img_non, 'img_non')
        self._tensor(img_ocl, 'img_ocl')
        n = img_non.size(0)
        if tuple(img_non.shape[1:]) != (3, 112, 112) or img_ocl.shape != img_non.shape:
            raise RuntimeError('ffrnet_amd: training images must be [N,3,112,112] pairs')
        lab = self._labels(label, n, img_non.device)
        out = self._empty(5)
        self._call(self.lib.ffr_train_iteration, _ptr(img_non.contiguous()), _ptr(img_ocl.contiguous()), _ptr(lab), n,
                   _loss_weights(loss_weight), _ptr(out))
        return out

    def train_iteration_u8(self, img_non, img_ocl, label, flip=None, loss_weight=(1, 1, 1, 1)):
        """train_iteration from decoded images: img_non / img_ocl [N,112,112,3] uint8 HWC RGB (device); flip: optional
        bool / uint8 [N], one h-flip flag per PAIR (the clean and the occluded image are mirrored together)."""
        self._tensor(img_non, 'img_non', torch.uint8, ('N', 112, 112, 3), _U8_HINT)
        self._tensor(img_ocl, 'img_ocl', torch.uint8, ('N', 112, 112, 3), _U8_HINT)
        n = img_non.size(0)
        if img_ocl.shape != img_non.shape:
            raise RuntimeError('ffrnet_amd: training images must be [N,112,112,3] pairs, got %s and %s'
                               % (list(img_non.shape), list(img_ocl.shape)))
        fl = self._flags(flip, n)
        lab = self._labels(label, n, img_non.device)
        out = self._empty(5)
        self._call(self.lib.ffr_train_iteration_u8, _ptr(img_non.contiguous()), _ptr(img_ocl.contiguous()), _ptr(fl), _ptr(lab),
                   n, _loss_weights(loss_weight), _ptr(out))
        return out

    def train_buckets(self):
        """[(offset, count)] of the gradient buckets in the order the backward finishes them, with their ids."""
        n = C.c_int(0)
        off = (C.c_size_t * 6)()
        order = (C.c_int * 5)()
        self._ck(self.lib.ffr_train_buckets(self._h, C.byref(n), off, order))
        return [(int(order[k]), int(off[order[k]]), int(off[order[k] + 1] - off[order[k]])) for k in range(n.value)]

    def train_bucket_wait(self, i, stream):
        """`stream` (torch.cuda.Stream) waits on the device until the enqueued backward has finished bucket i."""
        self._ck(self.lib.ffr_train_bucket_wait(self._h, int(i), C.c_void_p(stream.cuda_stream)))

    def train_option(self, name, value):
        self._ck(self.lib.ffr_train_option(self._h, name.encode(), int(value)))

    def train_debug(self, name, shape, slot=0):
        out = torch.empty(shape, dtype=torch.float32)
        self._ck(self.lib.ffr_train_debug_copy(self._h, slot, name.encode(), C.c_void_p(out.data_ptr()), out.numel()))
        return out

    def train_wgrad_plan(self):
        """The weight-gradient launches of the most recent backward (training backward or op_convlayer_train), in launch
        order (test hook): [{layer, name, path ('plain-taps9' | 'plain-taps1' | 'batched'), rows, cout_pad, Ng, nbatch, nkt,
        splits, kt_per_split, full_tiles, tail_splits, tail_kt, accumulate}], layer = position in the backward."""
        n = C.c_int(0)
        self._ck(self.lib.ffr_train_wgrad_plan(self._h, None, 0, C.byref(n)))
        arr = (WgradLaunch * max(n.value, 1))()
        self._ck(self.lib.ffr_train_wgrad_plan(self._h, arr, n.value, C.byref(n)))
        out = []
        for i in range(n.value):
            r = arr[i]
            d = {f: getattr(r, f) for f, _ in WgradLaunch._fields_[1:]}
            d.update(layer=i, name=r.name.decode(), path=WGRAD_PATHS[r.path])
            out.append(d)
        return out

    def train_adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_value=1.0):
        self._call(self.lib.ffr_train_adam_step, lr, betas[0], betas[1], eps, weight_decay, clip_value)

    def encoder_trunk_nhwc(self, x, n_blocks, out=None):
        """Stem + the first n_blocks bottlenecks -> the NHWC activation (test hook); `out` = a preallocated result."""
        self._tensor(x, 'x')
        x = x.contiguous()
        n, _, h, w = x.shape
        chans, div = 64, 1
        from .synth import ir_blocks
        for cin, depth, stride in ir_blocks(getattr(self, 'num_layers', 50))[:n_blocks]:
            chans, div = depth, div * stride
        if out is None:
            out = self._empty(n, h // div, w // div, chans)
        else:
            self._tensor(out, 'out', shape=(n, h // div, w // div, chans))
            if not out.is_contiguous():
                raise RuntimeError('ffrnet_amd: out must be contiguous')
        self._call(self.lib.ffr_encoder_trunk_nhwc, _ptr(x), n, h, w, n_blocks, _ptr(out))
        return out

    def recnet_debug(self, featmap, image=0):
        """RecNet's internals (test hook); ss_channel0 / M_channel0 are those of image `image`."""
        self._tensor(featmap, 'input', shape=('N', 512, 7, 7))
        featmap = featmap.contiguous()
        n = featmap.size(0)
        o = dict(ss_space=self._empty(n, 49, 49), M_space=self._empty(n, 49, 49), feat_space=self._empty(n, 512, 7, 7),
                 feat_channel_raw=self._empty(n, 512, 7, 7), feat_channel=self._empty(n, 512, 7, 7),
                 ss_channel0=self._empty(512, 512), M_channel0=self._empty(512, 512))
        self._call(self.lib.ffr_recnet_debug, _ptr(featmap), n, *[_ptr(t) for t in o.values()], int(image))
        return o


class GraphedEmbed(object):
    """hipGraph replay of Engine.embed for a fixed batch size (small batches are launch bound: one
    forward is ~190 launches).  The whole forward is enqueued by ONE ffr_embed call that neither
    allocates nor synchronises once the workspace is reserved, so it captures as is.
        g = GraphedEmbed(engine, n);  f_new, f = g(x)       # x[n,3,112,112] on the device
    The returned tensors are the graph's static outputs (overwritten by the next call)."""

    def __init__(self, engine, n):
        self.engine, self.n = engine, n
        dev = engine.device
        self.x = torch.zeros((n, 3, 112, 112), device=dev, dtype=torch.float32)
        self.f_new = torch.empty((n, 512), device=dev, dtype=torch.float32)
        self.f = torch.empty((n, 512), device=dev, dtype=torch.float32)
        self.captures = 0
        self._capture()

    def _capture(self):
        """The graph holds raw pointers into the handle's workspace and packed weights: it is only valid for the
        allocation generation it was captured in (Engine.generation())."""
        engine, dev = self.engine, self.engine.device
        engine.reserve(self.n)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                      # warm-up outside the capture
            engine.embed(self.x, out=(self.f_new, self.f))
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            engine.embed(self.x, out=(self.f_new, self.f))
        self.generation = engine.generation()
        self.captures += 1

    def __call__(self, x):
        if isinstance(x, torch.Tensor) and x.dtype == torch.uint8:
            raise RuntimeError('GraphedEmbed replays the fp32 forward only: for uint8 images call Engine.embed_u8 (or '
                               'pass engine.embed to lfw.calculate_distance)')
        _check_dev(x, 'x', (3, 112, 112), device=self.engine.device)
        if x.size(0) != self.n:
            raise RuntimeError('GraphedEmbed was captured for batch %d, got %d' % (self.n, x.size(0)))
        if self.engine.generation() != self.generation:
            # a larger batch, a weight reload or ffr_train_init re-allocated what the graph points into
            self._capture()
        self.x.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.f_new, self.f
