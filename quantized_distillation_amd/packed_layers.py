"""nn.Linear and nn.Embedding that run straight from the packed level indices of a quantized weight (libqd_infer.so,
include/qd_infer.h): a layer keeps `bits` bits per weight + (alpha, beta) per bucket on the device and never holds the
fp32 tensor.  The format is codec.pack_uniform's for the 2-D weight; the value of a weight is bit for bit what
PackedUniform.unpack() gives.

Inference only: the outputs carry no grad_fn.  To train or fine-tune, take `unpack()` -- an ordinary nn.Linear /
nn.Embedding with the fake-quantized fp32 weights.  HIP device only: there is no CPU path.
"""
import collections.abc

import torch
from torch import nn

from . import _infer, _lib, codec


def _levels_and_bits(s, bits):
    s = _lib.level_count(s)
    if s > 256:
        raise ValueError('the packed format holds at most 256 levels, got s = %d' % s)
    bits = codec.min_bits_for_levels(s) if bits is None else bits
    if not isinstance(bits, int) or isinstance(bits, bool) or not 1 <= bits <= 8 or s > (1 << bits):
        raise ValueError('bits must be an integer from 1 to 8 and hold s levels (s <= 2**bits), got bits = %r for s = %d' % (bits, s))
    return s, bits


def _require_device(t, what):
    if not t.is_cuda:
        raise NotImplementedError('%s: packed layers are implemented for tensors on a HIP device only (got %s); '
                                  'unpack() gives an ordinary module that runs anywhere' % (what, t.device))


class _PackedModule(nn.Module):
    """The packed weight of one 2-D tensor as registered buffers (so .to(device) moves it) + what describes the format."""

    def __init__(self, packed, bias=None):
        super().__init__()
        if not isinstance(packed, codec.PackedUniform):
            raise TypeError('packed must be a codec.PackedUniform (codec.pack_uniform of the 2-D weight), got %r' % type(packed))
        if len(packed.shape) != 2:
            raise ValueError('the packed weight must be 2-D [rows, cols], got shape %s' % (tuple(packed.shape),))
        self.s, self.bits = _levels_and_bits(packed.s, packed.bits)
        bucket = packed.bucket_size
        if bucket is not None and (not isinstance(bucket, int) or isinstance(bucket, bool) or bucket <= 0):
            raise ValueError('bucket_size must be a positive integer or None, got %r' % (bucket,))
        self.bucket_size = bucket
        self.rows, self.cols = int(packed.shape[0]), int(packed.shape[1])
        n = self.rows * self.cols
        nb = 1 if (bucket is None or n < bucket) else -(-n // bucket)
        if packed.packed.dtype != torch.uint8 or packed.packed.numel() != (n * self.bits + 7) // 8:
            raise ValueError('packed must hold ceil(rows cols bits / 8) = %d uint8, got %d %s'
                             % ((n * self.bits + 7) // 8, packed.packed.numel(), packed.packed.dtype))
        for name, t in (('alpha', packed.alpha), ('beta', packed.beta)):
            if t.dtype != torch.float32 or t.numel() != nb:
                raise ValueError('%s must hold one float32 per bucket (%d), got %d %s' % (name, nb, t.numel(), t.dtype))
        if bias is not None:
            if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
                raise TypeError('bias must be a float32 tensor or None')
            if bias.dim() != 1 or bias.numel() != self.rows:
                raise ValueError('bias must have shape [%d], got %s' % (self.rows, tuple(bias.shape)))
            if bias.device != packed.packed.device:
                raise ValueError('bias lives on %s, the packed weight on %s' % (bias.device, packed.packed.device))
            bias = bias.detach().contiguous()
        self.register_buffer('packed', packed.packed.contiguous())
        self.register_buffer('alpha', packed.alpha.contiguous().view(-1))
        self.register_buffer('beta', packed.beta.contiguous().view(-1))
        self.register_buffer('bias', bias)

    @property
    def nbytes(self):
        """Bytes this layer keeps on the device: PackedUniform.nbytes (+ the fp32 bias)."""
        return self.as_packed_uniform().nbytes + (0 if self.bias is None else 4 * self.bias.numel())

    @property
    def fp32_nbytes(self):
        """Bytes of the fp32 layer it stands for."""
        return 4 * self.rows * self.cols + (0 if self.bias is None else 4 * self.bias.numel())

    def as_packed_uniform(self):
        return codec.PackedUniform(self.packed, self.alpha, self.beta, (self.rows, self.cols), self.s, self.bucket_size, self.bits)

    def _weight(self):
        _require_device(self.packed, type(self).__name__ + '.unpack')
        if _lib.on_other_device(self.packed):
            with torch.cuda.device(self.packed.device):
                return self.as_packed_uniform().unpack()
        return self.as_packed_uniform().unpack()

    def _format_args(self):
        return (self.packed.data_ptr(), self.alpha.data_ptr(), self.beta.data_ptr(), self.rows, self.cols, self.bucket_size or 0,
                self.s, self.bits)

    def extra_repr(self):
        return 'rows=%d, cols=%d, s=%d, bits=%d, bucket_size=%r, bias=%s' % (self.rows, self.cols, self.s, self.bits, self.bucket_size,
                                                                            self.bias is not None)


def _pack_weight(weight, s, bucket_size, bits, what):
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32:
        raise TypeError('%s: the weight must be a float32 tensor' % what)
    if weight.dim() != 2:
        raise ValueError('%s: the weight must be 2-D, got shape %s' % (what, tuple(weight.shape)))
    s, bits = _levels_and_bits(s, bits)
    if bucket_size is not None and (not isinstance(bucket_size, int) or isinstance(bucket_size, bool) or bucket_size <= 0):
        raise ValueError('Bucket size must be an integer and strictly positive. Pass None if you want to avoid using buckets')
    _require_device(weight, what)
    return codec.pack_uniform(weight.detach(), s, bucket_size, bits)


class PackedLinear(_PackedModule):
    """y = x W^T + bias with W[N, K] read from its packed level indices (qdi_linear_packed_f32)."""

    @classmethod
    def from_linear(cls, linear, s, bucket_size=256, bits=None):
        """Quantize the weight of an nn.Linear with `s` levels per bucket; bits=None takes codec.min_bits_for_levels(s)."""
        if not isinstance(linear, nn.Linear):
            raise TypeError('from_linear takes an nn.Linear, got %r' % type(linear))
        pk = _pack_weight(linear.weight, s, bucket_size, bits, 'PackedLinear.from_linear')
        return cls(pk, None if linear.bias is None else linear.bias.detach().clone())

    @property
    def in_features(self):
        return self.cols

    @property
    def out_features(self):
        return self.rows

    def forward(self, x):
        if not isinstance(x, torch.Tensor):
            raise TypeError('x must be a torch.Tensor, got %r' % type(x))
        if x.dtype != torch.float32:
            raise TypeError('x must be float32, got %s' % x.dtype)
        if x.dim() < 1 or x.shape[-1] != self.cols:
            raise ValueError('x must have a last dimension of %d (in_features), got shape %s' % (self.cols, tuple(x.shape)))
        _require_device(self.packed, 'PackedLinear')
        _require_device(x, 'PackedLinear')
        if x.device != self.packed.device:
            raise ValueError('x lives on %s, the packed weight on %s' % (x.device, self.packed.device))
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError('PackedLinear is inference only and does not differentiate through x; run under torch.no_grad(), '
                               'or train with unpack(), the nn.Linear of the fake-quantized weights')
        if _lib.on_other_device(x):
            with torch.cuda.device(x.device):
                return self.forward(x)
        xc = x.detach().contiguous()
        m = int(torch.Size(x.shape[:-1]).numel())
        y = torch.empty(tuple(x.shape[:-1]) + (self.rows,), dtype=torch.float32, device=x.device)
        _infer.check(_infer.load().qdi_linear_packed_f32(*self._format_args(), xc.data_ptr(), m,
                                                         None if self.bias is None else self.bias.data_ptr(), y.data_ptr(),
                                                         _lib.stream_ptr()))
        return y

    def unpack(self):
        """An ordinary nn.Linear holding the fake-quantized fp32 weights (and the bias)."""
        w = self._weight()
        lin = nn.Linear(self.cols, self.rows, bias=self.bias is not None, device=w.device)
        with torch.no_grad():
            lin.weight.copy_(w)
            if self.bias is not None:
                lin.bias.copy_(self.bias)
        return lin


class PackedEmbedding(_PackedModule):
    """out[...] = W[indices[...]] with W[num_embeddings, dim] read from its packed level indices (qdi_embedding_packed_f32).
    An index outside [0, num_embeddings) gives a row of NaN."""

    def __init__(self, packed):
        super().__init__(packed, None)

    @classmethod
    def from_embedding(cls, emb, s, bucket_size=256, bits=None):
        if not isinstance(emb, nn.Embedding):
            raise TypeError('from_embedding takes an nn.Embedding, got %r' % type(emb))
        if emb.max_norm is not None:
            raise ValueError('an nn.Embedding with max_norm renormalises its rows on every lookup: it has no packed form')
        return cls(_pack_weight(emb.weight, s, bucket_size, bits, 'PackedEmbedding.from_embedding'))

    @property
    def num_embeddings(self):
        return self.rows

    @property
    def embedding_dim(self):
        return self.cols

    def forward(self, indices):
        if not isinstance(indices, torch.Tensor):
            raise TypeError('indices must be a torch.Tensor, got %r' % type(indices))
        if indices.dtype != torch.int64:
            raise TypeError('indices must be int64, got %s' % indices.dtype)
        _require_device(self.packed, 'PackedEmbedding')
        _require_device(indices, 'PackedEmbedding')
        if indices.device != self.packed.device:
            raise ValueError('indices live on %s, the packed weight on %s' % (indices.device, self.packed.device))
        if _lib.on_other_device(indices):
            with torch.cuda.device(indices.device):
                return self.forward(indices)
        ic = indices.contiguous()
        out = torch.empty(tuple(indices.shape) + (self.cols,), dtype=torch.float32, device=indices.device)
        _infer.check(_infer.load().qdi_embedding_packed_f32(*self._format_args(), ic.data_ptr(), ic.numel(), out.data_ptr(),
                                                            _lib.stream_ptr()))
        return out

    def unpack(self):
        """An ordinary nn.Embedding holding the fake-quantized fp32 weights."""
        w = self._weight()
        emb = nn.Embedding(self.rows, self.cols, device=w.device)
        with torch.no_grad():
            emb.weight.copy_(w)
        return emb


def pack_modules(model, s, bucket_size=256, bits=None, skip=()):
    """Replace every nn.Linear and nn.Embedding of `model` in place by its packed form.  skip: names (model.named_modules())
    left as they are; s: the level count, or a mapping from module name to it (every replaced module must be in it).
    Returns {name: (fp32_bytes, packed_bytes)} of what was replaced."""
    skip = set(skip)
    todo = [(name, mod) for name, mod in model.named_modules() if isinstance(mod, (nn.Linear, nn.Embedding)) and name not in skip]
    unknown = skip - {name for name, _ in model.named_modules()}
    if unknown:
        raise ValueError('skip names no module of the model: %s' % sorted(unknown))
    per_name = isinstance(s, collections.abc.Mapping)
    if per_name:
        missing = [name for name, _ in todo if name not in s]
        if missing:
            raise ValueError('s is a mapping and has no entry for: %s' % missing)
    plan = [(name, mod, _levels_and_bits(s[name] if per_name else s, bits)) for name, mod in todo]      # every s checked before any change
    report = {}
    for name, mod, (s_i, bits_i) in plan:
        if name == '':
            raise ValueError('the model itself is an nn.Linear / nn.Embedding: use from_linear / from_embedding')
        new = (PackedLinear.from_linear if isinstance(mod, nn.Linear) else PackedEmbedding.from_embedding)(mod, s_i, bucket_size, bits_i)
        parent_name, _, leaf = name.rpartition('.')
        parent = model.get_submodule(parent_name) if parent_name else model
        setattr(parent, leaf, new)
        report[name] = (new.fp32_nbytes, new.nbytes)
    return report
