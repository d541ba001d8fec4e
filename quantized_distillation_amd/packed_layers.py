"""nn.Linear, nn.Embedding, nn.Conv2d, nn.LSTMCell, nn.LSTM, nn.GRUCell, nn.GRU and a Luong global-attention step that run straight from the packed level indices
of a quantized weight (libqd_infer.so, include/qd_infer.h; for many rows of x libqd_infer_mm.so, include/qd_infer_mm.h;
convolutions libqd_infer_conv.so, include/qd_infer_conv.h; LSTM steps libqd_infer_rnn.so, include/qd_infer_rnn.h; GRU steps
libqd_infer_gru.so, include/qd_infer_gru.h; a global-attention step libqd_infer_attn.so, include/qd_infer_attn.h; the generator with its
log-softmax and top-k libqd_infer_gen.so, include/qd_infer_gen.h): a layer keeps `bits` bits per
weight + (alpha, beta) per bucket on the device and never holds the fp32 tensor.  The format is codec.pack_uniform's for the
2-D weight; the value of a weight is bit for bit what PackedUniform.unpack() gives.

Inference only: the outputs carry no grad_fn.  To train or fine-tune, take `unpack()` -- an ordinary nn.Linear /
nn.Embedding / nn.Conv2d / nn.LSTMCell / nn.LSTM / nn.GRUCell / nn.GRU with the fake-quantized fp32 weights.  HIP device only: there is no CPU path.
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


def _batched_from(value):
    if value is not None and (not isinstance(value, int) or isinstance(value, bool) or value < 1):
        raise ValueError('batched_from must be None or an integer >= 1 (the number of rows of x from which calls take the '
                         'batched MFMA kernel), got %r' % (value,))
    return value


class PackedLinear(_PackedModule):
    """y = x W^T + bias with W[N, K] read from its packed level indices.

    batched_from=None: every call is qdi_linear_packed_f32 (libqd_infer.so: one wave per output row, made for a handful of rows
    of x).  batched_from=M0: calls with at least M0 rows of x (the product of x's leading dimensions) are
    qdm_linear_packed_f32 (libqd_infer_mm.so, loaded on first use: fp32 MFMA, the weights decoded once per 64 rows of x).  Both
    keep the bound of include/qd_infer.h; their summation orders differ, so their results differ in the last bits."""

    def __init__(self, packed, bias=None, batched_from=None):
        batched_from = _batched_from(batched_from)
        super().__init__(packed, bias)
        self.batched_from = batched_from

    @classmethod
    def from_linear(cls, linear, s, bucket_size=256, bits=None, batched_from=None):
        """Quantize the weight of an nn.Linear with `s` levels per bucket; bits=None takes codec.min_bits_for_levels(s)."""
        if not isinstance(linear, nn.Linear):
            raise TypeError('from_linear takes an nn.Linear, got %r' % type(linear))
        batched_from = _batched_from(batched_from)
        pk = _pack_weight(linear.weight, s, bucket_size, bits, 'PackedLinear.from_linear')
        return cls(pk, None if linear.bias is None else linear.bias.detach().clone(), batched_from)

    def extra_repr(self):
        return super().extra_repr() + ', batched_from=%r' % (self.batched_from,)

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
        args = self._format_args() + (xc.data_ptr(), m, None if self.bias is None else self.bias.data_ptr(), y.data_ptr(), _lib.stream_ptr())
        if self.batched_from is not None and m >= self.batched_from:
            from . import _infer_mm                                       # libqd_infer_mm.so: on first use only
            _infer_mm.check(_infer_mm.load().qdm_linear_packed_f32(*args))
        else:
            _infer.check(_infer.load().qdi_linear_packed_f32(*args))
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


def _pair(value, what, least):
    """An int or a pair of ints >= least, as (h, w)."""
    pair = (value, value) if isinstance(value, int) else tuple(value) if isinstance(value, (tuple, list)) else None
    if pair is None or len(pair) != 2 or any(not isinstance(v, int) or isinstance(v, bool) or v < least for v in pair):
        raise ValueError('%s must be an integer >= %d or a pair of them, got %r' % (what, least, value))
    return pair


def _check_conv2d(conv, what):
    """The nn.Conv2d that have a packed form: groups 1, dilation 1, zero padding given in numbers."""
    if not isinstance(conv, nn.Conv2d):                                  # nn.ConvTranspose2d is no nn.Conv2d
        raise ValueError('%s takes an nn.Conv2d (transposed convolutions have no packed form), got %r' % (what, type(conv)))
    if conv.groups != 1 or tuple(conv.dilation) != (1, 1):
        raise ValueError('%s: groups = %d, dilation = %s: only groups 1 and dilation 1 have a packed form' % (what, conv.groups, tuple(conv.dilation)))
    if conv.padding_mode != 'zeros' or isinstance(conv.padding, str):
        raise ValueError('%s: padding_mode %r, padding %r: only zero padding given in numbers has a packed form'
                         % (what, conv.padding_mode, conv.padding))


class PackedConv2d(_PackedModule):
    """y = conv2d(x, W) + bias with W[cout, cin, kh, kw] read from its packed level indices, the 2-D weight [cout, cin kh kw]
    (qdc_conv2d_packed_f32, libqd_infer_conv.so, loaded on first use: an implicit GEMM on fp32 MFMA).  Zero padding, dilation 1,
    groups 1; x and y are contiguous NCHW."""

    def __init__(self, packed, kernel_size, stride=1, padding=0, bias=None):
        geometry = _pair(kernel_size, 'kernel_size', 1), _pair(stride, 'stride', 1), _pair(padding, 'padding', 0)
        super().__init__(packed, bias)
        self.kernel_size, self.stride, self.padding = geometry
        taps = self.kernel_size[0] * self.kernel_size[1]
        if self.cols % taps:
            raise ValueError('the packed weight has %d columns, no multiple of kh kw = %d' % (self.cols, taps))
        self.in_channels, self.out_channels = self.cols // taps, self.rows

    @classmethod
    def from_conv2d(cls, conv, s, bucket_size=256, bits=None):
        """Quantize the weight of an nn.Conv2d, seen as [cout, cin kh kw], with `s` levels per bucket: the buckets are flat, so
        this is the packed form of what the training quantizer makes of conv.weight."""
        _check_conv2d(conv, 'PackedConv2d.from_conv2d')
        pk = _pack_weight(conv.weight.reshape(conv.out_channels, -1), s, bucket_size, bits, 'PackedConv2d.from_conv2d')
        return cls(pk, tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding), None if conv.bias is None else conv.bias.detach().clone())

    def extra_repr(self):
        return '%d, %d, kernel_size=%s, stride=%s, padding=%s, ' % (self.in_channels, self.out_channels, self.kernel_size, self.stride,
                                                                   self.padding) + super().extra_repr()

    def forward(self, x):
        if not isinstance(x, torch.Tensor):
            raise TypeError('x must be a torch.Tensor, got %r' % type(x))
        if x.dtype != torch.float32:
            raise TypeError('x must be float32, got %s' % x.dtype)
        (kh, kw), (sh, sw), (ph, pw) = self.kernel_size, self.stride, self.padding
        if x.dim() != 4 or x.shape[1] != self.in_channels or x.shape[2] + 2 * ph < kh or x.shape[3] + 2 * pw < kw:
            raise ValueError('x must be [N, %d, H, W] with H + %d >= %d and W + %d >= %d, got shape %s'
                             % (self.in_channels, 2 * ph, kh, 2 * pw, kw, tuple(x.shape)))
        _require_device(self.packed, 'PackedConv2d')
        _require_device(x, 'PackedConv2d')
        if x.device != self.packed.device:
            raise ValueError('x lives on %s, the packed weight on %s' % (x.device, self.packed.device))
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError('PackedConv2d is inference only and does not differentiate through x; run under torch.no_grad(), '
                               'or train with unpack(), the nn.Conv2d of the fake-quantized weights')
        if _lib.on_other_device(x):
            with torch.cuda.device(x.device):
                return self.forward(x)
        xc = x.detach().contiguous()                                     # channels_last is copied to NCHW
        n, _, h, w = x.shape
        y = torch.empty((n, self.rows, (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1), dtype=torch.float32, device=x.device)
        from . import _infer_conv                                        # libqd_infer_conv.so: on first use only
        _infer_conv.check(_infer_conv.load().qdc_conv2d_packed_f32(
            self.packed.data_ptr(), self.alpha.data_ptr(), self.beta.data_ptr(), self.rows, self.in_channels, kh, kw, self.bucket_size or 0,
            self.s, self.bits, xc.data_ptr(), n, h, w, sh, sw, ph, pw, None if self.bias is None else self.bias.data_ptr(), y.data_ptr(),
            _lib.stream_ptr()))
        return y

    def unpack(self):
        """An ordinary nn.Conv2d holding the fake-quantized fp32 weights (and the bias), same stride and padding."""
        w = self._weight()
        conv = nn.Conv2d(self.in_channels, self.rows, self.kernel_size, self.stride, self.padding, bias=self.bias is not None, device=w.device)
        with torch.no_grad():
            conv.weight.copy_(w.view_as(conv.weight))
            if self.bias is not None:
                conv.bias.copy_(self.bias)
        return conv


def _check_rnn_tensor(t, what, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor, got %r' % (what, type(t)))
    if t.dtype != torch.float32:
        raise TypeError('%s must be float32, got %s' % (what, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('%s must have shape %s, got %s' % (what, tuple(shape), tuple(t.shape)))


def _check_rnn_call(module, tensors):
    """Devices and grad mode of a PackedLSTMCell / PackedLSTM / PackedGRUCell / PackedGRU call: everything on the weight's HIP device, nothing to differentiate."""
    name = type(module).__name__
    _require_device(module._device_of(), name)
    for t in tensors:
        _require_device(t, name)
        if t.device != module._device_of().device:
            raise ValueError('an input lives on %s, the packed weights on %s' % (t.device, module._device_of().device))
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError('%s is inference only and does not differentiate through its inputs; run under torch.no_grad(), '
                               'or train with unpack(), the torch module of the fake-quantized weights' % name)


class _PackedRecurrentCell(nn.Module):
    """What PackedLSTMCell and PackedGRUCell share: two packed weights `ih` and `hh` (each a _PackedModule with its bias)."""

    @classmethod
    def _from_weights(cls, w_ih, w_hh, b_ih, b_hh, s, bucket_size, bits, what):
        return cls(_pack_weight(w_ih, s, bucket_size, bits, what), _pack_weight(w_hh, s, bucket_size, bits, what),
                   None if b_ih is None else b_ih.detach().clone(), None if b_hh is None else b_hh.detach().clone())

    @property
    def nbytes(self):
        """Bytes this cell keeps on the device: both packed weights and the fp32 biases."""
        return self.ih.nbytes + self.hh.nbytes

    @property
    def fp32_nbytes(self):
        """Bytes of the fp32 cell it stands for."""
        return self.ih.fp32_nbytes + self.hh.fp32_nbytes

    def extra_repr(self):
        return '%d, %d, bias_ih=%s, bias_hh=%s' % (self.input_size, self.hidden_size, self.ih.bias is not None, self.hh.bias is not None)

    def _device_of(self):
        return self.hh.packed

    def _weight_args(self, part):
        return (part.packed.data_ptr(), part.alpha.data_ptr(), part.beta.data_ptr(), part.bucket_size or 0, part.s, part.bits)


class _PackedRecurrent(nn.Module):
    """What PackedLSTM and PackedGRU share: `cells`, one packed cell per layer and direction."""

    @property
    def nbytes(self):
        return sum(cl.nbytes for cl in self.cells)

    @property
    def fp32_nbytes(self):
        return sum(cl.fp32_nbytes for cl in self.cells)

    def extra_repr(self):
        return '%d, %d, num_layers=%d, bidirectional=%s, batch_first=%s' % (self.input_size, self.hidden_size, self.num_layers,
                                                                            self.bidirectional, self.batch_first)

    def _device_of(self):
        return self.cells[0]._device_of()


class PackedLSTMCell(_PackedRecurrentCell):
    """nn.LSTMCell with W_ih [4 hidden, input] and W_hh [4 hidden, hidden] read from their packed level indices, each packed as a
    tensor of its own (qdr_lstm_cell_packed_f32, libqd_infer_rnn.so, loaded on first use: both products on fp32 MFMA into one
    accumulator and the gate arithmetic in the same launch).  forward(x, (h, c)) -> (h', c'); without a state, zeros."""

    def __init__(self, packed_ih, packed_hh, bias_ih=None, bias_hh=None):
        super().__init__()
        self.ih = _PackedModule(packed_ih, bias_ih)
        self.hh = _PackedModule(packed_hh, bias_hh)
        self.input_size, self.hidden_size = self.ih.cols, self.hh.cols
        if self.hh.rows != 4 * self.hidden_size or self.ih.rows != self.hh.rows:
            raise ValueError('the packed weights must be [4 hidden, input] and [4 hidden, hidden], got [%d, %d] and [%d, %d]'
                             % (self.ih.rows, self.ih.cols, self.hh.rows, self.hh.cols))
        if self.ih.packed.device != self.hh.packed.device:
            raise ValueError('W_ih lives on %s, W_hh on %s' % (self.ih.packed.device, self.hh.packed.device))

    @classmethod
    def from_lstm_cell(cls, cell, s, bucket_size=256, bits=None):
        """Quantize weight_ih and weight_hh of an nn.LSTMCell, each as its own tensor, with `s` levels per bucket."""
        if not isinstance(cell, nn.LSTMCell):
            raise TypeError('from_lstm_cell takes an nn.LSTMCell, got %r' % type(cell))
        return cls._from_weights(cell.weight_ih, cell.weight_hh, cell.bias_ih if cell.bias else None, cell.bias_hh if cell.bias else None,
                                 s, bucket_size, bits, 'PackedLSTMCell.from_lstm_cell')

    def _step(self, x, pre, h, c, h_out, c_out):
        """One qdr_lstm_cell_packed_f32 on contiguous tensors of the current device: cell mode (x) or pre mode (pre)."""
        from . import _infer_rnn                                         # libqd_infer_rnn.so: on first use only
        ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
        ih = self._weight_args(self.ih) if pre is None else (None, None, None, 0, 0, 0)
        _infer_rnn.check(_infer_rnn.load().qdr_lstm_cell_packed_f32(
            *ih, *self._weight_args(self.hh), self.hidden_size, self.input_size, ptr(x), ptr(pre), h.data_ptr(), c.data_ptr(), h.shape[0],
            ptr(self.ih.bias) if pre is None else None, ptr(self.hh.bias), h_out.data_ptr(), c_out.data_ptr(), None, _lib.stream_ptr()))

    def forward(self, x, state=None):
        _check_rnn_tensor(x, 'x')
        if x.dim() not in (1, 2) or x.shape[-1] != self.input_size:
            raise ValueError('x must be [batch, %d] or [%d], got shape %s' % (self.input_size, self.input_size, tuple(x.shape)))
        lead = tuple(x.shape[:-1])
        if state is not None:
            if not isinstance(state, (tuple, list)) or len(state) != 2:
                raise TypeError('the state must be a pair (h, c), got %r' % type(state))
            for t, name in zip(state, ('h', 'c')):
                _check_rnn_tensor(t, name, lead + (self.hidden_size,))
        _check_rnn_call(self, (x,) + tuple(state or ()))
        if _lib.on_other_device(x):
            with torch.cuda.device(x.device):
                return self.forward(x, state)
        batch = x.shape[0] if x.dim() == 2 else 1
        xc = x.detach().contiguous().view(batch, self.input_size)
        if state is None:
            h = c = torch.zeros(batch, self.hidden_size, dtype=torch.float32, device=x.device)
        else:
            h, c = (t.detach().contiguous().view(batch, self.hidden_size) for t in state)
        h_out, c_out = torch.empty_like(h), torch.empty_like(c)
        self._step(xc, None, h, c, h_out, c_out)
        return h_out.view(lead + (self.hidden_size,)), c_out.view(lead + (self.hidden_size,))

    def unpack(self):
        """An ordinary nn.LSTMCell holding the fake-quantized fp32 weights (and the biases)."""
        w_ih, w_hh = self.ih._weight(), self.hh._weight()
        if (self.ih.bias is None) != (self.hh.bias is None):
            raise ValueError('an nn.LSTMCell has both biases or none; this cell has one')
        cell = nn.LSTMCell(self.input_size, self.hidden_size, bias=self.hh.bias is not None, device=w_hh.device)
        with torch.no_grad():
            cell.weight_ih.copy_(w_ih)
            cell.weight_hh.copy_(w_hh)
            if self.hh.bias is not None:
                cell.bias_ih.copy_(self.ih.bias)
                cell.bias_hh.copy_(self.hh.bias)
        return cell


def _check_lstm(lstm, what):
    if not isinstance(lstm, nn.LSTM):
        raise TypeError('%s takes an nn.LSTM, got %r' % (what, type(lstm)))
    if lstm.proj_size != 0:
        raise ValueError('%s: an nn.LSTM with proj_size = %d has no packed form' % (what, lstm.proj_size))


class PackedLSTM(_PackedRecurrent):
    """nn.LSTM (any num_layers, either direction count, either batch_first; no projections, no dropout: inference) from packed
    weights.  cells: one PackedLSTMCell per layer and direction, layer-major (layer 0 forward, layer 0 reverse, layer 1 ...).
    Per layer and direction the input projection of ALL time steps is one qdm_linear_packed_f32 (libqd_infer_mm.so) with bias_ih,
    then T launches of qdr_lstm_cell_packed_f32 in pre mode: step t reads h of the step before from the layer's output and
    writes its own there, c is updated in place.  The reverse direction is the same kernel walked from T - 1 down.  A
    bidirectional layer writes each direction's steps to a buffer of its own and concatenates them once per layer.
    forward(x, hx=None) -> (output, (h_n, c_n)) in nn.LSTM's shapes."""

    def __init__(self, cells, bidirectional=False, batch_first=False):
        super().__init__()
        cells = list(cells)
        dirs = 2 if bidirectional else 1
        if not cells or len(cells) % dirs or any(not isinstance(cl, PackedLSTMCell) for cl in cells):
            raise ValueError('cells must be a non-empty list of PackedLSTMCell, one per layer and direction')
        self.bidirectional, self.batch_first = bool(bidirectional), bool(batch_first)
        self.num_layers = len(cells) // dirs
        self.input_size, self.hidden_size = cells[0].input_size, cells[0].hidden_size
        for k, cl in enumerate(cells):
            want = self.input_size if k < dirs else dirs * self.hidden_size
            if cl.hidden_size != self.hidden_size or cl.input_size != want:
                raise ValueError('cell %d must be (input %d, hidden %d), got (%d, %d)' % (k, want, self.hidden_size, cl.input_size, cl.hidden_size))
            if cl._device_of().device != cells[0]._device_of().device:
                raise ValueError('the cells live on different devices')
        self.cells = nn.ModuleList(cells)

    @classmethod
    def from_lstm(cls, lstm, s, bucket_size=256, bits=None):
        """Quantize every weight_ih_l* / weight_hh_l* of an nn.LSTM, each as its own tensor, with `s` levels per bucket."""
        _check_lstm(lstm, 'PackedLSTM.from_lstm')
        cells = []
        for layer in range(lstm.num_layers):
            for sfx in ('', '_reverse')[:2 if lstm.bidirectional else 1]:
                get = lambda name: getattr(lstm, '%s_l%d%s' % (name, layer, sfx))           # noqa: E731
                cells.append(PackedLSTMCell._from_weights(get('weight_ih'), get('weight_hh'), get('bias_ih') if lstm.bias else None,
                                                          get('bias_hh') if lstm.bias else None, s, bucket_size, bits, 'PackedLSTM.from_lstm'))
        return cls(cells, lstm.bidirectional, lstm.batch_first)

    def forward(self, x, hx=None):
        if isinstance(x, nn.utils.rnn.PackedSequence):
            raise TypeError('PackedLSTM takes a padded tensor, not a PackedSequence')
        _check_rnn_tensor(x, 'x')
        if x.dim() not in (2, 3) or x.shape[-1] != self.input_size:
            raise ValueError('x must be [T, batch, %d] ([batch, T, %d] with batch_first) or [T, %d], got shape %s'
                             % (self.input_size, self.input_size, self.input_size, tuple(x.shape)))
        dirs = 2 if self.bidirectional else 1
        batched = x.dim() == 3
        seq = x if not batched else x.transpose(0, 1) if self.batch_first else x
        T, batch = seq.shape[0], seq.shape[1] if batched else 1
        if T == 0:
            raise ValueError('x holds no time step')
        state_shape = (self.num_layers * dirs,) + ((batch,) if batched else ()) + (self.hidden_size,)
        if hx is not None:
            if not isinstance(hx, (tuple, list)) or len(hx) != 2:
                raise TypeError('hx must be a pair (h_0, c_0), got %r' % type(hx))
            for t, name in zip(hx, ('h_0', 'c_0')):
                _check_rnn_tensor(t, name, state_shape)
        _check_rnn_call(self, (x,) + tuple(hx or ()))
        if _lib.on_other_device(x):
            with torch.cuda.device(x.device):
                return self.forward(x, hx)
        from . import _infer_mm                                          # libqd_infer_mm.so: the input projections
        H = self.hidden_size
        full = (self.num_layers * dirs, batch, H)
        if hx is None:
            h0 = torch.zeros(full, dtype=torch.float32, device=x.device)
            c_n = torch.zeros(full, dtype=torch.float32, device=x.device)
        else:
            h0, c_n = hx[0].detach().contiguous().view(full), hx[1].detach().clone(memory_format=torch.contiguous_format).view(full)
        h_n = torch.empty(full, dtype=torch.float32, device=x.device)
        inp = seq.detach().contiguous().view(T, batch, self.input_size)
        for layer in range(self.num_layers):
            outs = []
            for d in range(dirs):
                k = layer * dirs + d
                cl = self.cells[k]
                pre = torch.empty(T, batch, 4 * H, dtype=torch.float32, device=x.device)
                _infer_mm.check(_infer_mm.load().qdm_linear_packed_f32(
                    *cl.ih._format_args(), inp.data_ptr(), T * batch, None if cl.ih.bias is None else cl.ih.bias.data_ptr(), pre.data_ptr(),
                    _lib.stream_ptr()))
                out = torch.empty(T, batch, H, dtype=torch.float32, device=x.device)
                order = range(T - 1, -1, -1) if d else range(T)
                h = h0[k]
                for t in order:
                    cl._step(None, pre[t], h, c_n[k], out[t], c_n[k])
                    h = out[t]
                h_n[k].copy_(h)
                outs.append(out)
            inp = outs[0] if dirs == 1 else torch.cat(outs, dim=2)
        if not batched:
            return inp.view(T, dirs * H), (h_n.view(state_shape), c_n.view(state_shape))
        return (inp.transpose(0, 1) if self.batch_first else inp), (h_n, c_n)

    def unpack(self):
        """An ordinary nn.LSTM holding the fake-quantized fp32 weights (and the biases)."""
        biased = self.cells[0].hh.bias is not None
        if any((cl.ih.bias is not None) != biased or (cl.hh.bias is not None) != biased for cl in self.cells):
            raise ValueError('an nn.LSTM has every bias or none; these cells differ')
        lstm = nn.LSTM(self.input_size, self.hidden_size, self.num_layers, bias=biased, batch_first=self.batch_first,
                       bidirectional=self.bidirectional, device=self._device_of().device)
        dirs = 2 if self.bidirectional else 1
        with torch.no_grad():
            for k, cl in enumerate(self.cells):
                sfx = '_l%d%s' % (k // dirs, '_reverse' if k % dirs else '')
                getattr(lstm, 'weight_ih' + sfx).copy_(cl.ih._weight())
                getattr(lstm, 'weight_hh' + sfx).copy_(cl.hh._weight())
                if biased:
                    getattr(lstm, 'bias_ih' + sfx).copy_(cl.ih.bias)
                    getattr(lstm, 'bias_hh' + sfx).copy_(cl.hh.bias)
        return lstm


class PackedGRUCell(_PackedRecurrentCell):
    """nn.GRUCell with W_ih [3 hidden, input] and W_hh [3 hidden, hidden] read from their packed level indices, each packed as a
    tensor of its own (qdg_gru_cell_packed_f32, libqd_infer_gru.so, loaded on first use: both products on fp32 MFMA, kept as two
    sums because the reset gate multiplies the recurrent one, and the gate arithmetic in the same launch).
    forward(x, h=None) -> h'; without a state, zeros."""

    def __init__(self, packed_ih, packed_hh, bias_ih=None, bias_hh=None):
        super().__init__()
        self.ih = _PackedModule(packed_ih, bias_ih)
        self.hh = _PackedModule(packed_hh, bias_hh)
        self.input_size, self.hidden_size = self.ih.cols, self.hh.cols
        if self.hh.rows != 3 * self.hidden_size or self.ih.rows != self.hh.rows:
            raise ValueError('the packed weights must be [3 hidden, input] and [3 hidden, hidden], got [%d, %d] and [%d, %d]'
                             % (self.ih.rows, self.ih.cols, self.hh.rows, self.hh.cols))
        if self.ih.packed.device != self.hh.packed.device:
            raise ValueError('W_ih lives on %s, W_hh on %s' % (self.ih.packed.device, self.hh.packed.device))

    @classmethod
    def from_gru_cell(cls, cell, s, bucket_size=256, bits=None):
        """Quantize weight_ih and weight_hh of an nn.GRUCell, each as its own tensor, with `s` levels per bucket."""
        if not isinstance(cell, nn.GRUCell):
            raise TypeError('from_gru_cell takes an nn.GRUCell, got %r' % type(cell))
        return cls._from_weights(cell.weight_ih, cell.weight_hh, cell.bias_ih if cell.bias else None, cell.bias_hh if cell.bias else None,
                                 s, bucket_size, bits, 'PackedGRUCell.from_gru_cell')

    def _step(self, x, pre, h, h_out):
        """One qdg_gru_cell_packed_f32 on contiguous tensors of the current device: cell mode (x) or pre mode (pre)."""
        from . import _infer_gru                                         # libqd_infer_gru.so: on first use only
        ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
        ih = self._weight_args(self.ih) if pre is None else (None, None, None, 0, 0, 0)
        _infer_gru.check(_infer_gru.load().qdg_gru_cell_packed_f32(
            *ih, *self._weight_args(self.hh), self.hidden_size, self.input_size, ptr(x), ptr(pre), h.data_ptr(), h.shape[0],
            ptr(self.ih.bias) if pre is None else None, ptr(self.hh.bias), h_out.data_ptr(), None, _lib.stream_ptr()))

    def forward(self, x, h=None):
        _check_rnn_tensor(x, 'x')
        if x.dim() not in (1, 2) or x.shape[-1] != self.input_size:
            raise ValueError('x must be [batch, %d] or [%d], got shape %s' % (self.input_size, self.input_size, tuple(x.shape)))
        lead = tuple(x.shape[:-1])
        if h is not None:
            _check_rnn_tensor(h, 'h', lead + (self.hidden_size,))
        _check_rnn_call(self, (x,) if h is None else (x, h))
        if _lib.on_other_device(x):
            with torch.cuda.device(x.device):
                return self.forward(x, h)
        batch = x.shape[0] if x.dim() == 2 else 1
        xc = x.detach().contiguous().view(batch, self.input_size)
        if h is None:
            hc = torch.zeros(batch, self.hidden_size, dtype=torch.float32, device=x.device)
        else:
            hc = h.detach().contiguous().view(batch, self.hidden_size)
        h_out = torch.empty_like(hc)
        self._step(xc, None, hc, h_out)
        return h_out.view(lead + (self.hidden_size,))

    def unpack(self):
        """An ordinary nn.GRUCell holding the fake-quantized fp32 weights (and the biases)."""
        w_ih, w_hh = self.ih._weight(), self.hh._weight()
        if (self.ih.bias is None) != (self.hh.bias is None):
            raise ValueError('an nn.GRUCell has both biases or none; this cell has one')
        cell = nn.GRUCell(self.input_size, self.hidden_size, bias=self.hh.bias is not None, device=w_hh.device)
        with torch.no_grad():
            cell.weight_ih.copy_(w_ih)
            cell.weight_hh.copy_(w_hh)
            if self.hh.bias is not None:
                cell.bias_ih.copy_(self.ih.bias)
                cell.bias_hh.copy_(self.hh.bias)
        return cell


class PackedGRU(_PackedRecurrent):
    """nn.GRU (any num_layers, either direction count, either batch_first; no dropout: inference) from packed weights.  cells: one
    PackedGRUCell per layer and direction, layer-major (layer 0 forward, layer 0 reverse, layer 1 ...).  Per layer and direction
    the input projection of ALL time steps is one qdm_linear_packed_f32 (libqd_infer_mm.so) with bias_ih, then T launches of
    qdg_gru_cell_packed_f32 in pre mode: step t reads h of the step before from the layer's output and writes its own there.  The
    reverse direction is the same kernel walked from T - 1 down.  A bidirectional layer writes each direction's steps to a buffer
    of its own and concatenates them once per layer.  forward(x, hx=None) -> (output, h_n) in nn.GRU's shapes."""

    def __init__(self, cells, bidirectional=False, batch_first=False):
        super().__init__()
        cells = list(cells)
        dirs = 2 if bidirectional else 1
        if not cells or len(cells) % dirs or any(not isinstance(cl, PackedGRUCell) for cl in cells):
            raise ValueError('cells must be a non-empty list of PackedGRUCell, one per layer and direction')
        self.bidirectional, self.batch_first = bool(bidirectional), bool(batch_first)
        self.num_layers = len(cells) // dirs
        self.input_size, self.hidden_size = cells[0].input_size, cells[0].hidden_size
        for k, cl in enumerate(cells):
            want = self.input_size if k < dirs else dirs * self.hidden_size
            if cl.hidden_size != self.hidden_size or cl.input_size != want:
                raise ValueError('cell %d must be (input %d, hidden %d), got (%d, %d)' % (k, want, self.hidden_size, cl.input_size, cl.hidden_size))
            if cl._device_of().device != cells[0]._device_of().device:
                raise ValueError('the cells live on different devices')
        self.cells = nn.ModuleList(cells)

    @classmethod
    def from_gru(cls, gru, s, bucket_size=256, bits=None):
        """Quantize every weight_ih_l* / weight_hh_l* of an nn.GRU, each as its own tensor, with `s` levels per bucket."""
        if not isinstance(gru, nn.GRU):
            raise TypeError('PackedGRU.from_gru takes an nn.GRU, got %r' % type(gru))
        cells = []
        for layer in range(gru.num_layers):
            for sfx in ('', '_reverse')[:2 if gru.bidirectional else 1]:
                get = lambda name: getattr(gru, '%s_l%d%s' % (name, layer, sfx))            # noqa: E731
                cells.append(PackedGRUCell._from_weights(get('weight_ih'), get('weight_hh'), get('bias_ih') if gru.bias else None,
                                                         get('bias_hh') if gru.bias else None, s, bucket_size, bits, 'PackedGRU.from_gru'))
        return cls(cells, gru.bidirectional, gru.batch_first)

    def forward(self, x, hx=None):
        if isinstance(x, nn.utils.rnn.PackedSequence):
            raise TypeError('PackedGRU takes a padded tensor, not a PackedSequence')
        _check_rnn_tensor(x, 'x')
        if x.dim() not in (2, 3) or x.shape[-1] != self.input_size:
            raise ValueError('x must be [T, batch, %d] ([batch, T, %d] with batch_first) or [T, %d], got shape %s'
                             % (self.input_size, self.input_size, self.input_size, tuple(x.shape)))
        dirs = 2 if self.bidirectional else 1
        batched = x.dim() == 3
        seq = x if not batched else x.transpose(0, 1) if self.batch_first else x
        T, batch = seq.shape[0], seq.shape[1] if batched else 1
        if T == 0:
            raise ValueError('x holds no time step')
        state_shape = (self.num_layers * dirs,) + ((batch,) if batched else ()) + (self.hidden_size,)
        if hx is not None:
            _check_rnn_tensor(hx, 'h_0', state_shape)
        _check_rnn_call(self, (x,) if hx is None else (x, hx))
        if _lib.on_other_device(x):
            with torch.cuda.device(x.device):
                return self.forward(x, hx)
        from . import _infer_mm                                          # libqd_infer_mm.so: the input projections
        H = self.hidden_size
        full = (self.num_layers * dirs, batch, H)
        h0 = torch.zeros(full, dtype=torch.float32, device=x.device) if hx is None else hx.detach().contiguous().view(full)
        h_n = torch.empty(full, dtype=torch.float32, device=x.device)
        inp = seq.detach().contiguous().view(T, batch, self.input_size)
        for layer in range(self.num_layers):
            outs = []
            for d in range(dirs):
                k = layer * dirs + d
                cl = self.cells[k]
                pre = torch.empty(T, batch, 3 * H, dtype=torch.float32, device=x.device)
                _infer_mm.check(_infer_mm.load().qdm_linear_packed_f32(
                    *cl.ih._format_args(), inp.data_ptr(), T * batch, None if cl.ih.bias is None else cl.ih.bias.data_ptr(), pre.data_ptr(),
                    _lib.stream_ptr()))
                out = torch.empty(T, batch, H, dtype=torch.float32, device=x.device)
                h = h0[k]
                for t in (range(T - 1, -1, -1) if d else range(T)):
                    cl._step(None, pre[t], h, out[t])
                    h = out[t]
                h_n[k].copy_(h)
                outs.append(out)
            inp = outs[0] if dirs == 1 else torch.cat(outs, dim=2)
        if not batched:
            return inp.view(T, dirs * H), h_n.view(state_shape)
        return (inp.transpose(0, 1) if self.batch_first else inp), h_n

    def unpack(self):
        """An ordinary nn.GRU holding the fake-quantized fp32 weights (and the biases)."""
        biased = self.cells[0].hh.bias is not None
        if any((cl.ih.bias is not None) != biased or (cl.hh.bias is not None) != biased for cl in self.cells):
            raise ValueError('an nn.GRU has every bias or none; these cells differ')
        gru = nn.GRU(self.input_size, self.hidden_size, self.num_layers, bias=biased, batch_first=self.batch_first,
                     bidirectional=self.bidirectional, device=self._device_of().device)
        dirs = 2 if self.bidirectional else 1
        with torch.no_grad():
            for k, cl in enumerate(self.cells):
                sfx = '_l%d%s' % (k // dirs, '_reverse' if k % dirs else '')
                getattr(gru, 'weight_ih' + sfx).copy_(cl.ih._weight())
                getattr(gru, 'weight_hh' + sfx).copy_(cl.hh._weight())
                if biased:
                    getattr(gru, 'bias_ih' + sfx).copy_(cl.ih.bias)
                    getattr(gru, 'bias_hh' + sfx).copy_(cl.hh.bias)
        return gru


class PackedGlobalAttention(nn.Module):
    """One step of Luong global attention (the `dot` and `general` scores) with the output projection W_out [dim, 2 dim], and for
    `general` the input projection W_in [dim, dim], read from their packed level indices (libqd_infer_attn.so, include/qd_infer_attn.h,
    loaded on first use).  forward(query [batch, dim], memory [batch, S, dim], lengths=None, keys=None) -> (attn_h [batch, dim],
    align [batch, S]):

        q      = linear_in(query) where packed_in is given (`general`: one PackedLinear call), else query (`dot`)
        align  = softmax over s < lengths[b] of keys[b, s] . q[b], 0 from lengths[b] on      } qda_attn_context_f32, one launch;
        ctx    = sum_s align[b, s] memory[b, s]                                               } the padding is never read
        attn_h = tanh(W_out [ctx ; query] + bias_out)          qda_attn_out_packed_f32, one launch, no concatenation

    keys defaults to memory.  A decoder that projects the memory once per sentence (keys = attn_in(memory), then `dot`, as
    harness/models.py: Seq2SeqLSTM does) passes that projection as keys= with packed_in=None.  The concatenated operand is always
    the original query.  lengths: an int64 [batch] tensor; a row with lengths <= 0 is NaN.

    pack_modules does not build this layer -- there is no torch module to detect.  From the PackedLinear modules it leaves behind:
    PackedGlobalAttention(m.attn_out.as_packed_uniform(), bias_out=m.attn_out.bias), with packed_in=m.attn_in.as_packed_uniform()
    for the `general` form (a linear_in with a bias has no form here: the reference's has none).

    Not offered: the `mlp` (Bahdanau) score, coverage, multi-step queries [batch, T, dim] (call once per step) and PackedSequence
    inputs (pass the padded memory and lengths)."""

    def __init__(self, packed_out, packed_in=None, bias_out=None):
        super().__init__()
        self.out = _PackedModule(packed_out, bias_out)
        self.dim = self.out.rows
        if self.out.cols != 2 * self.dim:
            raise ValueError('packed_out must be [dim, 2 dim], got [%d, %d]' % (self.out.rows, self.out.cols))
        self.linear_in = None
        if packed_in is not None:
            self.linear_in = PackedLinear(packed_in)
            if (self.linear_in.rows, self.linear_in.cols) != (self.dim, self.dim):
                raise ValueError('packed_in must be [%d, %d], got [%d, %d]' % (self.dim, self.dim, self.linear_in.rows, self.linear_in.cols))
            if self.linear_in.packed.device != self.out.packed.device:
                raise ValueError('W_in lives on %s, W_out on %s' % (self.linear_in.packed.device, self.out.packed.device))

    @classmethod
    def from_linears(cls, linear_out, linear_in=None, s=None, bucket_size=256, bits=None):
        """Quantize the weights of the nn.Linear(2 dim, dim) behind tanh and, for `general`, of the bias-free nn.Linear(dim, dim) in
        front of the score, each as its own tensor, with `s` levels per bucket."""
        for lin, name in ((linear_out, 'linear_out'), (linear_in, 'linear_in')):
            if not isinstance(lin, nn.Linear) and not (lin is None and name == 'linear_in'):
                raise TypeError('from_linears: %s must be an nn.Linear, got %r' % (name, type(lin)))
        if s is None:
            raise TypeError('from_linears needs s, the number of levels')
        if linear_in is not None and linear_in.bias is not None:
            raise ValueError('from_linears: linear_in has a bias; the attention\'s input projection has none')
        what = 'PackedGlobalAttention.from_linears'
        return cls(_pack_weight(linear_out.weight, s, bucket_size, bits, what),
                   None if linear_in is None else _pack_weight(linear_in.weight, s, bucket_size, bits, what),
                   None if linear_out.bias is None else linear_out.bias.detach().clone())

    @property
    def nbytes(self):
        """Bytes this layer keeps on the device: the packed weights and the fp32 bias."""
        return self.out.nbytes + (0 if self.linear_in is None else self.linear_in.nbytes)

    @property
    def fp32_nbytes(self):
        """Bytes of the fp32 layers it stands for."""
        return self.out.fp32_nbytes + (0 if self.linear_in is None else self.linear_in.fp32_nbytes)

    def extra_repr(self):
        return '%d, score=%s, bias_out=%s' % (self.dim, 'dot' if self.linear_in is None else 'general', self.out.bias is not None)

    def _device_of(self):
        return self.out.packed

    def forward(self, query, memory, lengths=None, keys=None):
        if isinstance(memory, nn.utils.rnn.PackedSequence):
            raise TypeError('PackedGlobalAttention takes the padded memory and lengths, not a PackedSequence')
        _check_rnn_tensor(query, 'query')
        if query.dim() != 2 or query.shape[1] != self.dim:
            raise ValueError('query must be [batch, %d] (one step; call once per step for [batch, T, dim]), got shape %s' % (self.dim, tuple(query.shape)))
        _check_rnn_tensor(memory, 'memory')
        if memory.dim() != 3 or memory.shape[0] != query.shape[0] or memory.shape[2] != self.dim:
            raise ValueError('memory must be [%d, S, %d], got shape %s' % (query.shape[0], self.dim, tuple(memory.shape)))
        if keys is not None:
            _check_rnn_tensor(keys, 'keys', memory.shape)
        if lengths is not None:
            if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int64:
                raise TypeError('lengths must be an int64 tensor or None')
            if tuple(lengths.shape) != (query.shape[0],):
                raise ValueError('lengths must have shape [%d], got %s' % (query.shape[0], tuple(lengths.shape)))
        _check_rnn_call(self, [t for t in (query, memory, keys, lengths) if t is not None])
        if _lib.on_other_device(query):
            with torch.cuda.device(query.device):
                return self.forward(query, memory, lengths, keys)
        from . import _infer_attn                                        # libqd_infer_attn.so: on first use only
        lib = _infer_attn.load()
        batch, S = memory.shape[0], memory.shape[1]
        x = query.detach().contiguous()
        q = x if self.linear_in is None else self.linear_in(x)
        values = memory.detach().contiguous()
        ks = values if keys is None else keys.detach().contiguous()
        lens = None if lengths is None else lengths.contiguous()
        align = torch.empty(batch, S, dtype=torch.float32, device=x.device)
        ctx = torch.empty(batch, self.dim, dtype=torch.float32, device=x.device)
        attn_h = torch.empty(batch, self.dim, dtype=torch.float32, device=x.device)
        _infer_attn.check(lib.qda_attn_context_f32(q.data_ptr(), ks.data_ptr(), values.data_ptr(), None if lens is None else lens.data_ptr(),
                                                   batch, S, self.dim, align.data_ptr(), ctx.data_ptr(), _lib.stream_ptr()))
        o = self.out
        _infer_attn.check(lib.qda_attn_out_packed_f32(o.packed.data_ptr(), o.alpha.data_ptr(), o.beta.data_ptr(), o.bucket_size or 0, o.s, o.bits,
                                                      self.dim, ctx.data_ptr(), x.data_ptr(), batch, None if o.bias is None else o.bias.data_ptr(),
                                                      attn_h.data_ptr(), None, _lib.stream_ptr()))
        return attn_h, align

    def unpack(self):
        """(linear_out, linear_in or None): ordinary nn.Linear modules holding the fake-quantized fp32 weights (and the bias)."""
        w = self.out._weight()
        lin = nn.Linear(2 * self.dim, self.dim, bias=self.out.bias is not None, device=w.device)
        with torch.no_grad():
            lin.weight.copy_(w)
            if self.out.bias is not None:
                lin.bias.copy_(self.out.bias)
        return lin, None if self.linear_in is None else self.linear_in.unpack()


GeneratorOutput = collections.namedtuple('GeneratorOutput', 'log_probs lse top_values top_indices')


class PackedGenerator(_PackedModule):
    """The end of a decoder step -- generator = nn.Linear(dim, V), log_softmax and, in beam search, topk -- with W[V, dim] read
    from its packed level indices (qdn_generator_packed_f32, libqd_infer_gen.so, include/qd_infer_gen.h, loaded on first use: two
    launches, the logits reduced to (max, sum of exp, top-k) per panel of 64 words in the registers that hold them).

    forward(x [..., dim], topk=0, log_probs=True) -> GeneratorOutput(log_probs [..., V] or None, lse [...], top_values [..., topk]
    or None, top_indices [..., topk] int64 or None).  The logits have the bits of PackedLinear(batched_from=1) on the same weight;
    log_probs = logits - lse; the top k are ordered as torch.topk orders them (NaN first, ties to the lower index) and hold -inf
    and -1 from V on.  0 <= topk <= 16.  With log_probs=False the [m, V] array is never written.

    pack_modules does not build this layer -- a generator is an nn.Linear like any other.  From the PackedLinear it leaves behind:
    PackedGenerator(m.generator.as_packed_uniform(), bias=m.generator.bias)."""

    @classmethod
    def from_linear(cls, linear, s, bucket_size=256, bits=None):
        """Quantize the weight of the generator's nn.Linear with `s` levels per bucket; bits=None takes codec.min_bits_for_levels(s)."""
        if not isinstance(linear, nn.Linear):
            raise TypeError('from_linear takes an nn.Linear, got %r' % type(linear))
        pk = _pack_weight(linear.weight, s, bucket_size, bits, 'PackedGenerator.from_linear')
        return cls(pk, None if linear.bias is None else linear.bias.detach().clone())

    def forward(self, x, topk=0, log_probs=True):
        if not isinstance(x, torch.Tensor):
            raise TypeError('x must be a torch.Tensor, got %r' % type(x))
        if x.dtype != torch.float32:
            raise TypeError('x must be float32, got %s' % x.dtype)
        if x.dim() < 1 or x.shape[-1] != self.cols:
            raise ValueError('x must have a last dimension of %d, got shape %s' % (self.cols, tuple(x.shape)))
        if not isinstance(topk, int) or isinstance(topk, bool) or not 0 <= topk <= 16:
            raise ValueError('topk must be an integer from 0 to 16, got %r' % (topk,))
        _require_device(self.packed, 'PackedGenerator')
        _require_device(x, 'PackedGenerator')
        if x.device != self.packed.device:
            raise ValueError('x lives on %s, the packed weight on %s' % (x.device, self.packed.device))
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError('PackedGenerator is inference only and does not differentiate through x; run under torch.no_grad(), '
                               'or train with unpack(), the nn.Linear of the fake-quantized weights')
        if _lib.on_other_device(x):
            with torch.cuda.device(x.device):
                return self.forward(x, topk, log_probs)
        from . import _infer_gen                                         # libqd_infer_gen.so: on first use only
        lib = _infer_gen.load()
        xc = x.detach().contiguous()
        lead = tuple(x.shape[:-1])
        m = int(torch.Size(lead).numel())
        new = lambda shape, dtype=torch.float32: torch.empty(lead + shape, dtype=dtype, device=x.device)      # noqa: E731
        lse = new(())
        logp = new((self.rows,)) if log_probs else None
        top_val, top_idx = (new((topk,)), new((topk,), torch.int64)) if topk else (None, None)
        work = torch.empty(max(lib.qdn_generator_work_bytes(self.rows, m, topk), 4) // 4, dtype=torch.float32, device=x.device)
        ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
        _infer_gen.check(lib.qdn_generator_packed_f32(*self._format_args(), xc.data_ptr(), m, ptr(self.bias), lse.data_ptr(), ptr(logp), topk,
                                                      ptr(top_val), ptr(top_idx), work.data_ptr(), _lib.stream_ptr()))
        return GeneratorOutput(logp, lse, top_val, top_idx)

    def unpack(self):
        """An ordinary nn.Linear holding the fake-quantized fp32 weights (and the bias): the generator in front of log_softmax."""
        w = self._weight()
        lin = nn.Linear(self.cols, self.rows, bias=self.bias is not None, device=w.device)
        with torch.no_grad():
            lin.weight.copy_(w)
            if self.bias is not None:
                lin.bias.copy_(self.bias)
        return lin


def pack_modules(model, s, bucket_size=256, bits=None, skip=(), batched_from=None, conv=False, rnn=False):
    """Replace every nn.Linear and nn.Embedding of `model` -- with conv=True every nn.Conv2d, with rnn=True every nn.LSTM,
    nn.LSTMCell, nn.GRU and nn.GRUCell as well (an nn.LSTM with proj_size raises before anything is changed) -- in place by its
    packed form.  skip: names (model.named_modules()) left as they are; s: the level count, or a mapping from module name to it (every
    replaced module must be in it); batched_from: PackedLinear's, for every Linear replaced.  A Conv2d that has no packed form
    (groups, dilation, a padding mode) raises before anything is changed.  Returns {name: (fp32_bytes, packed_bytes)} of what
    was replaced."""
    batched_from = _batched_from(batched_from)
    skip = set(skip)
    kinds = (nn.Linear, nn.Embedding) + ((nn.Conv2d,) if conv else ()) + ((nn.LSTM, nn.LSTMCell, nn.GRU, nn.GRUCell) if rnn else ())
    todo = [(name, mod) for name, mod in model.named_modules() if isinstance(mod, kinds) and name not in skip]
    unknown = skip - {name for name, _ in model.named_modules()}
    if unknown:
        raise ValueError('skip names no module of the model: %s' % sorted(unknown))
    per_name = isinstance(s, collections.abc.Mapping)
    if per_name:
        missing = [name for name, _ in todo if name not in s]
        if missing:
            raise ValueError('s is a mapping and has no entry for: %s' % missing)
    plan = [(name, mod, _levels_and_bits(s[name] if per_name else s, bits)) for name, mod in todo]      # every s checked before any change
    for name, mod, _ in plan:
        if isinstance(mod, nn.Conv2d):
            _check_conv2d(mod, 'pack_modules: %s' % name)                 # and every convolution
        if isinstance(mod, nn.LSTM):
            _check_lstm(mod, 'pack_modules: %s' % name)                   # and every LSTM
    report = {}
    for name, mod, (s_i, bits_i) in plan:
        if name == '':
            raise ValueError('the model itself is an nn.Linear / nn.Embedding%s: use from_linear / from_embedding%s'
                             % ((' / nn.Conv2d', ' / from_conv2d') if conv else ('', '')))
        if isinstance(mod, nn.Linear):
            new = PackedLinear.from_linear(mod, s_i, bucket_size, bits_i, batched_from)
        elif isinstance(mod, nn.Conv2d):
            new = PackedConv2d.from_conv2d(mod, s_i, bucket_size, bits_i)
        elif isinstance(mod, nn.LSTM):
            new = PackedLSTM.from_lstm(mod, s_i, bucket_size, bits_i)
        elif isinstance(mod, nn.LSTMCell):
            new = PackedLSTMCell.from_lstm_cell(mod, s_i, bucket_size, bits_i)
        elif isinstance(mod, nn.GRU):
            new = PackedGRU.from_gru(mod, s_i, bucket_size, bits_i)
        elif isinstance(mod, nn.GRUCell):
            new = PackedGRUCell.from_gru_cell(mod, s_i, bucket_size, bits_i)
        else:
            new = PackedEmbedding.from_embedding(mod, s_i, bucket_size, bits_i)
        parent_name, _, leaf = name.rpartition('.')
        parent = model.get_submodule(parent_name) if parent_name else model
        setattr(parent, leaf, new)
        report[name] = (new.fp32_nbytes, new.nbytes)
    return report
