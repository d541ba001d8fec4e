"""One-launch forms of the per-parameter loops of the training steps: quantization of every parameter tensor of a
model (MultiTensorQuantizer), differentiable quantization (MultiTensorDiffQuant), the bucket-aware STE backward
(MultiTensorSTE) and the symbols a compressed checkpoint stores (MultiTensorSymbols).

The reference's training loops quantize parameter by parameter
(cnn_models/conv_forward_model.py:235-247, translation_models/model.py:247-258):

    for p in model.parameters():
        p.data = quantization.uniformQuantization(p.data, s, bucket_size=...)[0]

With 22-110 tensors per model, most of them tiny, that is launch/host bound.  Each class here builds a device table of
per-tensor descriptors {pointers, numel, work prefix} once (_DeviceTable) and runs the whole model with a single launch
per step (include/qd_hip.h); the results are bit-identical to the per-tensor calls.
"""
import ctypes
import numbers

import torch

from . import _lib


def _level_counts(s, tensors):
    """s of the uniform one-launch classes: an integer in [2, 2^31 - 1] for every tensor, or a sequence of them, one per tensor.  Returns
    (what `self.s` keeps: the int or a tuple, the list of tensors); only the list's length is looked at, no tensor is."""
    def one(v):
        return _lib.level_count(v)         # 's must be an integer >= 2 in the accepted range [2, 2^31 - 1]'
    if isinstance(s, numbers.Real) and not isinstance(s, bool):
        return one(s), tensors
    if isinstance(s, (str, bytes)) or not hasattr(s, '__iter__'):
        raise ValueError('s must be an integer >= 2, or a sequence of them with one entry per tensor')
    counts = tuple(one(v) for v in s)
    tensors = list(tensors)
    if len(counts) != len(tensors):
        raise ValueError('s has %d entries for %d tensors: need one per tensor' % (len(counts), len(tensors)))
    return counts, tensors


def _is_bucket_list(bucket_size):
    """bucket_size of the uniform one-launch classes is given per tensor: anything but None and a single number."""
    return bucket_size is not None and not isinstance(bucket_size, numbers.Real)


def _bucket_sizes(bucket_size, tensors):
    """A bucket_size given per tensor: a sequence of positive integers, one per tensor.  Returns (the tuple `self.bucket_size`
    keeps, the list of tensors); as in _level_counts only the list's length is looked at, no tensor is."""
    if isinstance(bucket_size, (str, bytes)) or not hasattr(bucket_size, '__iter__'):
        raise ValueError('bucket_size must be a positive integer, None, or a sequence of positive integers with one entry per '
                         'tensor')
    sizes = []
    for v in bucket_size:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 < v < 2 ** 63:
            raise ValueError('bucket_size entries must be positive integers, got %r' % (v,))
        sizes.append(int(v))
    tensors = list(tensors)
    if len(sizes) != len(tensors):
        raise ValueError('bucket_size has %d entries for %d tensors: need one per tensor' % (len(sizes), len(tensors)))
    return tuple(sizes), tensors


def per_channel_bucket_sizes(tensors):
    """The bucket_size list that gives every tensor one (alpha, beta) pair per output channel: the elements of t[0] for a
    tensor of two or more dimensions (a contiguous [out, ...] weight: buckets are flat runs, so a run of that length is a
    channel), and the whole tensor -- one bucket -- for a bias, a batch-norm vector or a scalar.  Never below 1, so that a
    tensor without elements keeps a valid entry.  Pure Python: no device, no tensor data is looked at."""
    sizes = []
    for t in tensors:
        if t.dim() >= 2:
            per = 1
            for extent in t.shape[1:]:
                per *= int(extent)
            sizes.append(max(per, 1))
        else:
            sizes.append(max(int(t.numel()), 1))
    return sizes


class _DeviceTable(object):
    """What the one-launch classes share: the argument check, the descriptor table on the device, and the launch on a table
    that is current.  A subclass names its descriptor type, says which tensors go into which field (_columns), calls the
    library's plan (_plan_table) and makes the launch calls."""
    _DESC = None           # the ctypes descriptor type (_lib.Qd*Desc)
    entry_point = None     # name of the C entry point the last launch went through (_entry)
    _WATCH = ()            # attributes holding the tensors a caller may rebind: the table is rebuilt when one of them moved

    def _adopt(self, first_contiguous=True, dtypes=None, **named):
        """named[what] = a sequence of tensors, one per tensor of the first sequence.  Returns them as lists of fp32 tensors on
        one HIP device (self.device), each with as many elements as its counterpart in the first list and contiguous (the
        first list too unless first_contiguous=False: tensors that are only read through a copy).  dtypes: {what: dtype} for
        the lists that hold another type than fp32 (the 16-bit outputs of MultiTensorQuantizer, the 16-bit gradients of
        MultiTensorSTE, either of MultiTensorDiffQuant)."""
        lists = [list(ts) for ts in named.values()]
        if not lists[0]:
            raise ValueError('no tensors')
        if any(len(ts) != len(lists[0]) for ts in lists):
            raise ValueError('%s: need one per tensor' % ', '.join(list(named)[1:]))
        for what, ts in zip(named, lists):
            for t, first in zip(ts, lists[0]):
                _lib.require_device_dtype(t, (dtypes or {}).get(what, torch.float32), what)
                if not t.is_contiguous() and (first_contiguous or ts is not lists[0]):
                    raise ValueError('%s must be contiguous' % what)
                if t.numel() != first.numel():
                    raise ValueError('%s must match the tensors in size' % what)
                if t.device != lists[0][0].device:
                    raise ValueError('all tensors of a multi-tensor launch must live on one device')
        self.device = lists[0][0].device
        return lists

    def _columns(self):
        """((descriptor field, list of tensors), ...); the first column gives the element counts."""
        raise NotImplementedError

    def _plan_table(self, host, n):
        """Call the library's plan on the host table (it fills the prefix fields), size the scratch; returns the tile count."""
        raise NotImplementedError

    def _held(self):
        return [t.data_ptr() for name in self._WATCH for t in getattr(self, name)]

    def _plan(self):
        cols = self._columns()
        self.n_tensors = n = len(cols[0][1])
        host = (self._DESC * n)()
        for i in range(n):
            for field, ts in cols:
                setattr(host[i], field, ts[i].data_ptr())
            host[i].n = cols[0][1][i].numel()
        self._tiles = self._plan_table(host, n)
        self._table = _lib.upload_struct(host, self.device)
        self._ptrs = self._held()

    def _launch(self, call, written=None, check_pointers=True):
        """_lib.check(call()) with the tensors' device current, on a table that points at the tensors held now.  `written`:
        the held tensors the launch writes through the table; with zero tiles they have no element and nothing is launched."""
        if check_pointers and self._held() != self._ptrs:
            self._plan()                   # a held tensor's storage was swapped (p.data rebound, set_, resize_)
        if written is not None and self._tiles <= 0:
            return written
        if _lib.on_other_device(self._table):
            with torch.cuda.device(self.device):
                return self._launch(call, written, check_pointers=False)
        _lib.check(call())
        if written is not None:
            _lib.mark_written(written)     # one native call bumps their version counters
        return written

    def _entry(self, name):
        """The C entry point a launch goes through; `entry_point` keeps the name of the last one taken."""
        self.entry_point = name
        return getattr(_lib.load(), name)

    def _bind_levels(self, s):
        """s as _level_counts returned it, once self.device is known.  Sets self.s, self._s (the one level count of the
        existing entry points: a scalar s, or a sequence whose entries are all equal -- such an object launches exactly what
        it always launched) and self._levels: None, or for a mixed sequence one int32 device array, entry i for tensor i.
        The array is the object's own and outlives every re-plan of the table (the entries go by position, not by pointer)."""
        self.s = s
        mixed = isinstance(s, tuple) and len(set(s)) > 1
        self._s = None if mixed else (s[0] if isinstance(s, tuple) else s)
        self._levels = torch.tensor(s, dtype=torch.int32, device=self.device) if mixed else None

    def _plan_buckets(self, plan, host, n):
        """_plan_table of an object whose bucket_size is a tuple, one entry per tensor: `plan` (qd_multi_buckets_plan /
        qd_multi_ste_buckets_plan) counts tensor i under entry i, and self._buckets becomes the int64 device array the launch
        reads -- built here, next to the table, from the values the plan was made with; returns the tile count."""
        sizes = (ctypes.c_int64 * n)(*self.bucket_size)
        tiles = ctypes.c_int64(0)
        _lib.check(plan(host, sizes, n, ctypes.byref(tiles)))
        self._buckets = torch.tensor(self.bucket_size, dtype=torch.int64, device=self.device)
        return int(tiles.value)

    def _own_levels(self, n):
        """The entry points that take a levels array take it always: one for equal entries too."""
        if self._levels is None:
            self._levels = torch.full((n,), self._s, dtype=torch.int32, device=self.device)


class MultiTensorQuantizer(_DeviceTable):
    """uniformQuantization(t, s, bucket_size=bucket_size, stochastic_rounding=..., max_element=...)[0] of every tensor, written
    to outputs[i], in one launch (qd_multi_uniform_f32; bucket_size=None: three, qd_multi_uniform_global_f32, and `alpha_beta`
    holds every tensor's (alpha, beta)).  With an option set the launch is qd_multi_uniform_opt_f32 /
    qd_multi_uniform_global_opt_f32; with none it is what it always was.

    stochastic_rounding: tensor i is rounded with seed0 + i, what the i-th call of the per-tensor loop draws
    (quant_functions.reserve_stochastic_seeds).  By default seed0 is a launch argument: quantize(seed=...) or the process
    counter, kept as `last_seed`; such a launch cannot be captured into a hipGraph (it would replay its draws).
    seed_on_device=True keeps seed0 in `seed_cell`, one int64 device word that reseed() writes and every quantize() advances
    by n_tensors on the launch's stream: nothing on the host is consulted, so the call can be captured and each replay
    draws anew -- launch r after a reseed uses seed0 + r * n_tensors + i (int64 wrap-around gives the bits of uint64).
    subtract_mean is not offered: call uniformQuantization per tensor for it.

    s: one level count for every tensor, or a sequence with one entry per tensor (per-layer bit widths: tensor i equals
    uniformQuantization(t_i, s[i], ...)); `self.s` keeps the int or a tuple.  A sequence of unequal entries is uploaded once
    as an int32 device array and every option combination launches qd_multi_uniform_levels_f32 /
    qd_multi_uniform_global_levels_f32; a scalar, or a sequence whose entries are all equal, launches what it always
    launched.  `entry_point` names the C entry point the last quantize() went through.

    bucket_size: None, one positive int for every tensor, or a sequence of positive ints with one entry per tensor (tensor i
    equals uniformQuantization(t_i, s_i, bucket_size=bucket_size[i], ...); per_channel_bucket_sizes(tensors) gives the list
    for one scale pair per output channel); `self.bucket_size` keeps None, the int or a tuple.  A sequence -- equal entries
    included -- always plans with qd_multi_buckets_plan and launches qd_multi_uniform_buckets_f32, whatever the options and
    the form of s; the int64 device array it reads is the object's own and is rebuilt with the table.  Every option above
    works as with one bucket size.  Not with fp16 / bf16 outputs: NotImplementedError.

    out_dtype: None (fp32 outputs: everything above, unchanged), torch.float16 or torch.bfloat16 -- fp32 masters quantized
    straight into a 16-bit model.  `outputs` may then be a list of tensors that are all fp16 or all bf16 (their dtype is
    enough: out_dtype may stay None), or None to have them allocated.  Element e of outputs[i] is the IEEE round-to-nearest-
    even conversion of what the fp32 launch writes -- outputs32[i].to(out_dtype), bit for bit -- in the same single launch
    (qd_multi_uniform_out16_f32; bucket_size=None: qd_multi_uniform_global_out16_f32), without an fp32 shadow and without the
    cast.  Every option and every form of s goes through that one pair of entry points; the object always owns a levels
    array.  The inputs stay fp32 and must not overlap the outputs.  `self.out_dtype` keeps the choice (None: fp32)."""
    _DESC = _lib.QdTensorDesc
    _WATCH = ('inputs', 'outputs')
    _OUT_KINDS = {torch.float16: 1, torch.bfloat16: 2}          # QD_OUT_F16, QD_OUT_BF16 (include/qd_hip.h)

    @classmethod
    def _output_dtype(cls, outputs, out_dtype):
        """The outputs' type from `outputs` (None, or a sequence of tensors) and `out_dtype`: None for fp32, else one of the
        two 16-bit types.  TypeError for anything else, for mixed outputs and for outputs that contradict out_dtype."""
        if out_dtype is not None and out_dtype != torch.float32 and out_dtype not in cls._OUT_KINDS:
            raise TypeError('out_dtype must be None, torch.float32, torch.float16 or torch.bfloat16, got %r' % (out_dtype,))
        have = out_dtype or torch.float32
        if outputs:
            for t in outputs:
                if not isinstance(t, torch.Tensor):
                    raise TypeError('outputs must be torch.Tensors, got %r' % type(t))
            kinds = {t.dtype for t in outputs}
            if len(kinds) > 1:
                raise TypeError('outputs must all have one dtype, got %s' % ', '.join(sorted(str(k) for k in kinds)))
            have = kinds.pop()
            if have != torch.float32 and have not in cls._OUT_KINDS:
                raise TypeError('outputs must be float32, float16 or bfloat16, got %s' % have)
            if out_dtype is not None and have != out_dtype:
                raise TypeError('outputs are %s but out_dtype is %s' % (have, out_dtype))
        return None if have == torch.float32 else have

    def __init__(self, tensors, s, bucket_size, outputs=None, stochastic_rounding=False, max_element=False,
                 subtract_mean=False, seed_on_device=False, out_dtype=None):
        per_tensor = _is_bucket_list(bucket_size)
        if not per_tensor and bucket_size is not None and (not isinstance(bucket_size, int) or bucket_size <= 0):
            raise ValueError('bucket_size must be a positive integer or None')
        s, tensors = _level_counts(s, tensors)
        if per_tensor:
            bucket_size, tensors = _bucket_sizes(bucket_size, tensors)
        if max_element is not False and (max_element is True or not isinstance(max_element, numbers.Number)):
            raise ValueError('maxElementAllowed must be a number')                  # as ScalingFunction, ref: :31-33
        if subtract_mean:
            raise NotImplementedError('MultiTensorQuantizer does not subtract the mean (a per-tensor, order-dependent sum): '
                                      'call quantization.uniformQuantization(t, s, subtract_mean=True, ...) per tensor')
        if seed_on_device and not stochastic_rounding:
            raise ValueError('seed_on_device=True needs stochastic_rounding=True')
        self.bucket_size = bucket_size
        self.stochastic_rounding = bool(stochastic_rounding)
        self.max_element = max_element
        self.seed_on_device = bool(seed_on_device)
        self.last_seed = None
        self.seed_cell = None
        outputs = None if outputs is None else list(outputs)
        self.out_dtype = self._output_dtype(outputs, out_dtype)
        self._buckets = None                       # the int64 device array of a per-tensor bucket_size (_plan_buckets)
        if per_tensor and self.out_dtype is not None:
            raise NotImplementedError('MultiTensorQuantizer: a bucket_size per tensor together with fp16 / bf16 outputs is not '
                                      'implemented: give one bucket_size, or fp32 outputs')
        if outputs is None:
            (self.inputs,) = self._adopt(tensors=tensors)
            self.outputs = [torch.empty_like(t, dtype=self.out_dtype) for t in self.inputs]
        else:
            self.inputs, self.outputs = self._adopt(tensors=tensors, outputs=outputs,
                                                    dtypes={'outputs': self.out_dtype or torch.float32})
        self._bind_levels(s)
        if self.out_dtype is not None and self._levels is None:     # the 16-bit entry points take the array, always
            self._levels = torch.full((len(self.inputs),), self._s, dtype=torch.int32, device=self.device)
        if per_tensor:                                              # ... and so does the per-tensor-bucket entry point
            self._own_levels(len(self.inputs))
        self._plan()
        if self.seed_on_device:
            self.seed_cell = torch.zeros(1, dtype=torch.int64, device=self.device)
            self.reseed()

    def _columns(self):
        return ('x', self.inputs), ('q', self.outputs)

    def _plan_table(self, host, n):
        if self.bucket_size is None:
            tiles = int(_lib.load().qd_multi_global_plan(host, n))
            self.alpha_beta = torch.empty(n, 2, dtype=torch.float32, device=self.device)     # per-tensor (alpha, beta)
            self._scratch = torch.empty(max(4, 2 * tiles), dtype=torch.float32, device=self.device)
        elif isinstance(self.bucket_size, tuple):
            tiles = self._plan_buckets(_lib.load().qd_multi_buckets_plan, host, n)
        else:
            tiles = int(_lib.load().qd_multi_plan(host, n, self.bucket_size))
        if tiles < 0:
            raise RuntimeError('qd_multi_plan failed')
        return tiles

    def _call(self):
        if self.bucket_size is None:
            return self._entry('qd_multi_uniform_global_f32')(
                self._table.data_ptr(), self.n_tensors, self._tiles, self._s, self.alpha_beta.data_ptr(),
                self._scratch.data_ptr(), self._scratch.numel() * 4, _lib.stream_ptr(self.device))
        return self._entry('qd_multi_uniform_f32')(self._table.data_ptr(), self.n_tensors, self._tiles, self.bucket_size, self._s,
                                                _lib.stream_ptr(self.device))

    def _call_opt(self, seed):
        clamp, me = (0, 0.0) if self.max_element is False else (1, float(self.max_element))
        cell = self.seed_cell.data_ptr() if self.seed_on_device else None
        if self.out_dtype is not None:             # 16-bit outputs: one pair of entry points for every option and every s
            kind = self._OUT_KINDS[self.out_dtype]
            if self.bucket_size is None:
                return self._entry('qd_multi_uniform_global_out16_f32')(
                    self._table.data_ptr(), self._levels.data_ptr(), self.n_tensors, self._tiles, kind, clamp, me,
                    int(self.stochastic_rounding), seed, cell, self.alpha_beta.data_ptr(), self._scratch.data_ptr(),
                    self._scratch.numel() * 4, _lib.stream_ptr(self.device))
            return self._entry('qd_multi_uniform_out16_f32')(
                self._table.data_ptr(), self._levels.data_ptr(), self.n_tensors, self._tiles, self.bucket_size, kind, clamp, me,
                int(self.stochastic_rounding), seed, cell, _lib.stream_ptr(self.device))
        if self._buckets is not None:              # a bucket size per tensor: one entry point for every option and every s
            return self._entry('qd_multi_uniform_buckets_f32')(
                self._table.data_ptr(), self._levels.data_ptr(), self._buckets.data_ptr(), self.n_tensors, self._tiles, clamp, me,
                int(self.stochastic_rounding), seed, cell, _lib.stream_ptr(self.device))
        if self._levels is not None:               # a level count per tensor: the one pair of entry points for every option
            if self.bucket_size is None:
                return self._entry('qd_multi_uniform_global_levels_f32')(
                    self._table.data_ptr(), self._levels.data_ptr(), self.n_tensors, self._tiles, clamp, me,
                    int(self.stochastic_rounding), seed, cell, self.alpha_beta.data_ptr(), self._scratch.data_ptr(),
                    self._scratch.numel() * 4, _lib.stream_ptr(self.device))
            return self._entry('qd_multi_uniform_levels_f32')(
                self._table.data_ptr(), self._levels.data_ptr(), self.n_tensors, self._tiles, self.bucket_size, clamp, me,
                int(self.stochastic_rounding), seed, cell, _lib.stream_ptr(self.device))
        if self.bucket_size is None:
            return self._entry('qd_multi_uniform_global_opt_f32')(
                self._table.data_ptr(), self.n_tensors, self._tiles, self._s, clamp, me, int(self.stochastic_rounding), seed,
                cell, self.alpha_beta.data_ptr(), self._scratch.data_ptr(), self._scratch.numel() * 4,
                _lib.stream_ptr(self.device))
        return self._entry('qd_multi_uniform_opt_f32')(
            self._table.data_ptr(), self.n_tensors, self._tiles, self.bucket_size, self._s, clamp, me,
            int(self.stochastic_rounding), seed, cell, _lib.stream_ptr(self.device))

    def reseed(self, seed0=None):
        """seed_on_device: write the device seed word; the next quantize() rounds tensor i with seed0 + i.  Default: the next
        n_tensors seeds of the process counter (quant_functions.reserve_stochastic_seeds).  Not inside a captured region."""
        if not self.seed_on_device:
            raise ValueError('reseed() needs seed_on_device=True')
        if seed0 is None:
            from .quantization.quant_functions import reserve_stochastic_seeds
            seed0 = reserve_stochastic_seeds(self.n_tensors)
        seed0 = int(seed0) & 0xFFFFFFFFFFFFFFFF
        self.seed_cell.fill_(seed0 - (1 << 64) if seed0 >= (1 << 63) else seed0)      # the same 64 bits as int64
        return seed0

    def quantize(self, check_pointers=True, seed=None):
        """Quantize all tensors (one launch).  Returns the list of output tensors.  seed: the by-value seed0 of a stochastic
        launch (default: the next n_tensors seeds of the process counter); kept as `last_seed`."""
        if seed is not None and (not self.stochastic_rounding or self.seed_on_device):
            raise ValueError('seed= is for stochastic_rounding=True with the seed passed by value (seed_on_device=False)')
        if not self.stochastic_rounding and self.max_element is False and self._levels is None:
            return self._launch(self._call, self.outputs, check_pointers)
        seed0 = 0
        if self.stochastic_rounding and not self.seed_on_device:
            from .quantization.quant_functions import next_stochastic_seed, reserve_stochastic_seeds
            if seed is None:
                seed = reserve_stochastic_seeds(self.n_tensors)       # raises during stream capture
            elif torch.cuda.is_current_stream_capturing():
                next_stochastic_seed()                                # the same RuntimeError: a by-value seed would be replayed
            self.last_seed = seed0 = int(seed) & 0xFFFFFFFFFFFFFFFF
        out = self._launch(lambda: self._call_opt(seed0), self.outputs, check_pointers)
        if self.seed_on_device:
            self.seed_cell.add_(self.n_tensors)        # on the launch's stream: the next launch, or replay, draws anew
        return out


class MultiTensorDiffQuant(_DeviceTable):
    """Both per-step sweeps of differentiable quantization over ALL tensors of a model in one
    launch each (qd_multi_nearest_f32 / qd_multi_point_grad_f32, include/qd_hip.h).

    The reference loops over the tensors calling nonUniformQuantization_variable.forward and
    .backward (cnn_models/conv_forward_model.py:524-545).  Here the scaled weights `u`, alpha and
    beta of every tensor are computed once (K2) and stay resident; `points` is ONE [ntensors, k]
    device tensor; every step
        forward():  points -> quantized weights written straight into `outputs[i]` (+ uint8 indices)
        backward(): gradients `grads[i]` -> grad of the points, [ntensors, k]
    Results are bit-identical (forward) / equal to rounding (backward) to the per-tensor calls.

    bucket_size: None (no buckets: one alpha / beta per tensor) or any positive int, as the per-tensor functions take them;
    num_points: 1 ... 256 (the index is a uint8).  Powers of two with at most 64 points are the tuned path; other bucket
    sizes and more points run the same launches through untuned instantiations.

    A 16-bit student over fp32 masters: `outputs` may be all torch.float16 or all torch.bfloat16 (its p.data), and,
    independently, `grads` may be all torch.float16 or all torch.bfloat16 (its p.grad).  The masters in `tensors`, the resident
    u, alpha, beta, `points` and the gradient of the points stay fp32.  forward() then writes the IEEE round-to-nearest-even
    conversion of what the fp32 launch writes -- outputs32[i].to(dtype), bit for bit, the same indices -- in the same single
    launch (qd_multi_nearest_out16_f32); backward() returns what the fp32 launch gives on grads[i].float(), bit for bit,
    whatever the alignment of the gradients (qd_multi_point_grad_in16_f32): no fp32 shadows, no torch._foreach_copy_ around
    the sweeps.  `self.out_dtype` / `self.grad_dtype` keep the 16-bit types (None: fp32, which launches what it always
    launched); rebind() takes tensors of the types given at construction.  `entry_point` names the C entry point of the last
    forward() / backward().
    """
    _DESC = _lib.QdDiffQuantDesc
    _WATCH = ('outputs', 'grads')
    _KINDS = {torch.float16: 1, torch.bfloat16: 2}              # QD_OUT_F16 = QD_GRAD_F16, QD_OUT_BF16 = QD_GRAD_BF16 (include/qd_hip.h)

    @classmethod
    def _one_dtype(cls, ts, what):
        """The one dtype of the list `ts` as out_dtype / grad_dtype keep it: None for fp32, else one of the two 16-bit types.
        TypeError for mixed lists and for any other dtype (what is no tensor at all is left to _adopt)."""
        kinds = {t.dtype for t in ts if isinstance(t, torch.Tensor)}
        if len(kinds) > 1:
            raise TypeError('%s must all have one dtype, got %s' % (what, ', '.join(sorted(str(k) for k in kinds))))
        have = kinds.pop() if kinds else torch.float32
        if have != torch.float32 and have not in cls._KINDS:
            raise TypeError('%s must be float32, float16 or bfloat16, got %s' % (what, have))
        return None if have == torch.float32 else have

    def _dtypes(self):
        return {'outputs': self.out_dtype or torch.float32, 'grads': self.grad_dtype or torch.float32}

    def __init__(self, tensors, outputs, grads, num_points, bucket_size):
        from .quantization.quant_functions import ScalingFunction
        if _is_bucket_list(bucket_size) and not isinstance(bucket_size, (str, bytes)) and hasattr(bucket_size, '__iter__'):
            raise NotImplementedError('MultiTensorDiffQuant with a bucket_size per tensor is not implemented: give one '
                                      'bucket_size (MultiTensorQuantizer and MultiTensorSTE take a sequence)')
        if bucket_size is not None and (type(bucket_size) is not int or bucket_size <= 0):      # as ScalingFunction (bool refused)
            raise ValueError('Bucket size must be an integer and strictly positive. '
                             'Pass None if you want to avoid using buckets')
        if type(num_points) is not int or not 1 <= num_points <= 256:
            raise ValueError('the multi-tensor diff-quant path supports 1..256 points per tensor (uint8 indices)')
        self.k, self.bucket_size = int(num_points), bucket_size
        # OWNING references: the device table below holds raw pointers into these tensors, so they are kept
        # alive here for the lifetime of the object.  A caller that rebinds `p.grad` (zero_grad(set_to_none=True))
        # does not free them; backward() then reads the buffers given HERE, which is what the pointer check guards.
        # (the tensors themselves are read once, by scale_down, which copies: any layout)
        tensors, outputs, grads = list(tensors), list(outputs), list(grads)
        self.out_dtype, self.grad_dtype = self._one_dtype(outputs, 'outputs'), self._one_dtype(grads, 'grads')
        tensors, self.outputs, self.grads = self._adopt(False, self._dtypes(), tensors=tensors, outputs=outputs, grads=grads)
        self.scalings, self.scaled, self.indices = [], [], []
        for t in tensors:
            sf = ScalingFunction('linear', False, False, bucket_size)
            self.scalings.append(sf)
            self.scaled.append(sf.scale_down(t).view(-1)[0:t.numel()].contiguous())
            self.indices.append(torch.empty(t.numel(), dtype=torch.uint8, device=self.device))
        self._plan()

    def _columns(self):
        return (('u', self.scaled), ('q', self.outputs), ('idx', self.indices), ('alpha', [sf.alpha for sf in self.scalings]),
                ('beta', [sf.beta for sf in self.scalings]), ('grad', self.grads))

    def _plan_table(self, host, n):
        rows = ctypes.c_int64(0)
        tiles = int(_lib.load().qd_multi_dq_plan(host, n, self.bucket_size or 0, ctypes.byref(rows)))
        if tiles < 0:
            raise RuntimeError('qd_multi_dq_plan failed')
        self._blocks = int(rows.value)             # partial rows of the gradient sweep
        self._scratch = torch.empty(max(1, self._blocks * self.k), dtype=torch.float32, device=self.device)
        return tiles

    def rebind(self, outputs=None, grads=None):
        """Point the device table at new output / gradient buffers (e.g. after the caller re-allocated
        its gradients) -- one small H2D copy.  The new tensors have the dtypes given at construction (TypeError otherwise)."""
        _, self.outputs, self.grads = self._adopt(True, self._dtypes(), scaled=self.scaled,
                                                  outputs=self.outputs if outputs is None else outputs,
                                                  grads=self.grads if grads is None else grads)
        self._plan()

    def forward(self, points):
        """points: [ntensors, k] fp32 device tensor, each row sorted.  Writes outputs[i] in place."""
        if points.shape != (self.n_tensors, self.k) or not points.is_contiguous():
            raise ValueError('points must be a contiguous [ntensors, k] tensor')
        if self.out_dtype is not None:
            return self._launch(lambda: self._entry('qd_multi_nearest_out16_f32')(
                self._table.data_ptr(), self.n_tensors, self._tiles, self.bucket_size or 0, points.data_ptr(), self.k,
                self._KINDS[self.out_dtype], _lib.stream_ptr(self.device)), self.outputs)
        return self._launch(lambda: self._entry('qd_multi_nearest_f32')(
            self._table.data_ptr(), self.n_tensors, self._tiles, self.bucket_size or 0, points.data_ptr(), self.k,
            _lib.stream_ptr(self.device)), self.outputs)

    def backward(self, out=None):
        """grad of the points from the gradient buffers given at construction: [ntensors, k]."""
        if out is None:
            out = torch.empty(self.n_tensors, self.k, dtype=torch.float32, device=self.device)
        if self.grad_dtype is not None:
            self._launch(lambda: self._entry('qd_multi_point_grad_in16_f32')(
                self._table.data_ptr(), self.n_tensors, self._blocks, self.bucket_size or 0, self.k,
                self._KINDS[self.grad_dtype], out.data_ptr(), self._scratch.data_ptr(), self._scratch.numel() * 4,
                _lib.stream_ptr(self.device)))
            return out
        self._launch(lambda: self._entry('qd_multi_point_grad_f32')(
            self._table.data_ptr(), self.n_tensors, self._blocks, self.bucket_size or 0, self.k, out.data_ptr(),
            self._scratch.data_ptr(), self._scratch.numel() * 4, _lib.stream_ptr(self.device)))
        return out


class MultiTensorSTE(_DeviceTable):
    """The 'complicated' straight-through backward (ste.ste_bucket_backward, K7) of ALL quantized tensors of a model in
    one launch (qd_multi_ste_backward_f32, include/qd_hip.h).

    The reference calls quantizeFunctions[idx].backward(p.grad.data) parameter by parameter
    (cnn_models/conv_forward_model.py:253-266).  Here the table of {weights, grad, out, numel} is built once;
        backward(): grads[i] -> outs[i] for every i (in place by default: outs = grads)
    `weights[i]` are the full-precision values the forward quantized.  Each result is bit-identical to
    ste.ste_bucket_backward(weights[i], grads[i], bucket_size, s, out=outs[i], tie_mode=tie_mode).
    s: one level count, or a sequence with one entry per tensor (s[i] in the call above), as MultiTensorQuantizer takes it:
    unequal entries launch qd_multi_ste_backward_levels_f32, anything else the entry point above (`entry_point` names the one
    the last backward() took).
    bucket_size: one positive int, or a sequence of positive ints with one entry per tensor (bucket_size[i] in the call above),
    as MultiTensorQuantizer takes it: a sequence always plans with qd_multi_ste_buckets_plan and launches
    qd_multi_ste_backward_buckets_f32 (fp32 gradients only: NotImplementedError with 16-bit ones).

    grads may instead be all torch.float16 or all torch.bfloat16 -- the p.grad of a 16-bit student over fp32 masters.
    `weights` stay fp32 and `outs` is a list of fp32 tensors (outs=None: allocated, one per gradient; there is no in-place form,
    the element sizes differ) that must not overlap the gradients or the weights.  Each result is bit-identical to the fp32
    object's on grads[i].float() -- the widening is exact and happens inside the one launch (qd_multi_ste_in16_plan,
    qd_multi_ste_backward_in16_f32), whatever the alignment of the gradients.  Every form of s goes through that entry point;
    the object always owns a levels array.  `self.grad_dtype` keeps the 16-bit type (None: fp32 gradients, which plan and
    launch what they always did).
    """
    _DESC = _lib.QdSteDesc
    _WATCH = ('weights', 'grads', 'outs')
    _GRAD_KINDS = {torch.float16: 1, torch.bfloat16: 2}         # QD_GRAD_F16, QD_GRAD_BF16 (include/qd_hip.h)

    @classmethod
    def _gradient_dtype(cls, grads):
        """None for fp32 gradients (and for whatever the fp32 path refuses itself), else the one 16-bit type of all of them.
        TypeError for 16-bit gradients mixed with anything else."""
        kinds = {t.dtype for t in grads if isinstance(t, torch.Tensor)}
        if not kinds & set(cls._GRAD_KINDS):
            return None
        if len(kinds) > 1 or not all(isinstance(t, torch.Tensor) for t in grads):
            raise TypeError('grads must all have one dtype, got %s' % ', '.join(sorted(str(k) for k in kinds)))
        return kinds.pop()

    def __init__(self, weights, grads, s, bucket_size, outs=None, tie_mode='reference'):
        if bucket_size is None:                                                         # ref: quant_functions.py:332-334
            raise NotImplementedError('Right now the code does not work with bucket_size None.'
                                      ' Not hard to modify though')
        per_tensor = _is_bucket_list(bucket_size)
        if not per_tensor and (isinstance(bucket_size, bool) or not isinstance(bucket_size, int) or bucket_size <= 0):
            raise ValueError('bucket_size must be a positive integer')
        s, weights = _level_counts(s, weights)
        if per_tensor:
            bucket_size, weights = _bucket_sizes(bucket_size, weights)
        if tie_mode not in ('reference', 'true_arg'):
            raise ValueError("tie_mode must be 'reference' or 'true_arg'")
        self.bucket_size = bucket_size
        self.tie_mode = 0 if tie_mode == 'reference' else 1
        grads = list(grads)
        self.grad_dtype = self._gradient_dtype(grads)
        self._buckets = None                       # the int64 device array of a per-tensor bucket_size (_plan_buckets)
        if per_tensor and self.grad_dtype is not None:
            raise NotImplementedError('MultiTensorSTE: a bucket_size per tensor together with fp16 / bf16 grads is not '
                                      'implemented: give one bucket_size, or fp32 gradients')
        # OWNING references: the device table holds raw pointers into these tensors
        if self.grad_dtype is not None:
            if outs is None:
                self.weights, self.grads = self._adopt(weights=weights, grad=grads, dtypes={'grad': self.grad_dtype})
                self.outs = [torch.empty(g.shape, dtype=torch.float32, device=g.device) for g in self.grads]
            else:
                self.weights, self.grads, self.outs = self._adopt(weights=weights, grad=grads, out=outs,
                                                                  dtypes={'grad': self.grad_dtype})
        elif outs is None:
            self.weights, self.grads = self._adopt(weights=weights, grad=grads)
            self.outs = self.grads
        else:
            self.weights, self.grads, self.outs = self._adopt(weights=weights, grad=grads, out=outs)
        self._bind_levels(s)
        if self.grad_dtype is not None and self._levels is None:    # the 16-bit entry point takes the array, always
            self._levels = torch.full((len(self.weights),), self._s, dtype=torch.int32, device=self.device)
        if per_tensor:                                              # ... and so does the per-tensor-bucket entry point
            self._own_levels(len(self.weights))
        self._plan()

    def _columns(self):
        return ('x', self.weights), ('g', self.grads), ('out', self.outs)

    def _plan_table(self, host, n):
        if isinstance(self.bucket_size, tuple):
            return self._plan_buckets(_lib.load().qd_multi_ste_buckets_plan, host, n)
        tiles = ctypes.c_int64(0)
        plan = _lib.load().qd_multi_ste_plan if self.grad_dtype is None else _lib.load().qd_multi_ste_in16_plan
        _lib.check(plan(host, n, self.bucket_size, ctypes.byref(tiles)))
        return int(tiles.value)

    def backward(self, check_pointers=True):
        """out = the bucket-aware STE gradient for every tensor (one launch).  Returns the list of outs."""
        if self.grad_dtype is not None:
            return self._launch(lambda: self._entry('qd_multi_ste_backward_in16_f32')(
                self._table.data_ptr(), self._levels.data_ptr(), self.n_tensors, self._tiles, self.bucket_size,
                self._GRAD_KINDS[self.grad_dtype], self.tie_mode, _lib.stream_ptr(self.device)), self.outs, check_pointers)
        if self._buckets is not None:
            return self._launch(lambda: self._entry('qd_multi_ste_backward_buckets_f32')(
                self._table.data_ptr(), self._levels.data_ptr(), self._buckets.data_ptr(), self.n_tensors, self._tiles,
                self.tie_mode, _lib.stream_ptr(self.device)), self.outs, check_pointers)
        if self._levels is not None:
            return self._launch(lambda: self._entry('qd_multi_ste_backward_levels_f32')(
                self._table.data_ptr(), self._levels.data_ptr(), self.n_tensors, self._tiles, self.bucket_size, self.tie_mode,
                _lib.stream_ptr(self.device)), self.outs, check_pointers)
        return self._launch(lambda: self._entry('qd_multi_ste_backward_f32')(
            self._table.data_ptr(), self.n_tensors, self._tiles, self.bucket_size, self._s, self.tie_mode,
            _lib.stream_ptr(self.device)), self.outs, check_pointers)


class MultiTensorSymbols(_DeviceTable):
    """What a compressed checkpoint stores of uniformly quantized tensors, for ALL tensors of a model in one launch
    (qd_multi_uniform_symbols_u8, include/qd_hip.h): the uint8 level index of every weight and the (alpha, beta) of every
    bucket, without the fp32 result.  Tensor i equals, bit for bit, the level indices, alpha and beta of
    uniformQuantization(t_i, s_i, bucket_size=bucket_size[i]) -- deterministic rounding, no clamp, no mean: the configuration
    save_compressed stores, and the call it makes for a bucket_size given per tensor.

    s: one level count or a sequence with one entry per tensor, each in 2 .. 256 (a symbol is a byte).
    bucket_size: one positive int for every tensor, or a sequence of positive ints with one entry per tensor
    (per_channel_bucket_sizes(tensors) gives the list for one scale pair per output channel); `self.bucket_size` keeps the
    tuple.  None -- whole-tensor scaling -- is not offered: NotImplementedError (the per-tensor call does it).
    symbols: optional list of contiguous uint8 device tensors of the tensors' sizes (any alignment); allocated by default.
    alpha_beta: optional pair of flat contiguous fp32 device tensors that receive alpha and beta (at least `buckets_total`
    elements each); allocated by default.

    `alpha` / `beta`: lists of fp32 views [nb_i] into the two flat tensors, in table order -- the layout of a compressed file's
    alpha and beta sections; `buckets_total` their total length.  encode() makes the one launch and returns `symbols`;
    `entry_point` names the C entry point once it ran."""
    _DESC = _lib.QdSymbolDesc
    _WATCH = ('inputs', 'symbols')
    ENTRY_POINT = 'qd_multi_uniform_symbols_u8'

    def __init__(self, tensors, s, bucket_size, symbols=None, alpha_beta=None):
        s, tensors = _level_counts(s, tensors)
        if any(v > 256 for v in (s if isinstance(s, tuple) else (s,))):
            raise ValueError('s must be an integer in 2 .. 256 (a symbol is one byte), or a sequence of them with one entry per '
                             'tensor')
        if bucket_size is None:
            raise NotImplementedError('MultiTensorSymbols needs a bucket_size: whole-tensor scaling (bucket_size=None) keeps the '
                                      'per-tensor call')
        if _is_bucket_list(bucket_size):
            bucket_size, tensors = _bucket_sizes(bucket_size, tensors)
        else:
            if isinstance(bucket_size, bool) or not isinstance(bucket_size, int) or bucket_size <= 0:
                raise ValueError('bucket_size must be a positive integer, or a sequence of positive integers with one entry per '
                                 'tensor')
            tensors = list(tensors)
            bucket_size = (bucket_size,) * len(tensors)
        self.bucket_size = bucket_size
        self._flat = None if alpha_beta is None else tuple(alpha_beta)
        if self._flat is not None and len(self._flat) != 2:
            raise ValueError('alpha_beta: a pair of flat float32 tensors')
        if symbols is None:
            (self.inputs,) = self._adopt(tensors=tensors)
            self.symbols = [torch.empty(t.numel(), dtype=torch.uint8, device=self.device) for t in self.inputs]
        else:
            self.inputs, self.symbols = self._adopt(tensors=tensors, symbols=symbols, dtypes={'symbols': torch.uint8})
        for t in self._flat or ():
            _lib.require_device_f32(t, 'alpha_beta')
            if not t.is_contiguous() or t.dim() != 1 or t.device != self.device:
                raise ValueError('alpha_beta: flat contiguous tensors on the device of the tensors')
        self._bind_levels(s)
        self._own_levels(len(self.inputs))
        self._plan()

    def _columns(self):
        return ('x', self.inputs), ('sym', self.symbols)

    def _plan_table(self, host, n):
        sizes = (ctypes.c_int64 * n)(*self.bucket_size)
        tiles, total = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.load().qd_multi_symbols_plan(host, sizes, n, ctypes.byref(tiles), ctypes.byref(total)))
        self._buckets = torch.tensor(self.bucket_size, dtype=torch.int64, device=self.device)
        self.buckets_total = int(total.value)
        if self._flat is None:             # the object's own (kept over a re-plan: the sizes cannot have changed)
            self._flat = tuple(torch.empty(max(self.buckets_total, 1), dtype=torch.float32, device=self.device) for _ in range(2))
        if any(t.numel() < self.buckets_total for t in self._flat):
            raise ValueError('alpha_beta: %d buckets need %d elements each' % (self.buckets_total, self.buckets_total))
        first = [host[i].first_bucket for i in range(n)] + [self.buckets_total]
        self.alpha, self.beta = ([t[first[i]:first[i + 1]] for i in range(n)] for t in self._flat)
        return int(tiles.value)

    def encode(self, check_pointers=True):
        """Symbols, alpha and beta of all tensors (one launch).  Returns the list of symbol tensors."""
        out = self._launch(lambda: self._entry(self.ENTRY_POINT)(
            self._table.data_ptr(), self._levels.data_ptr(), self._buckets.data_ptr(), self.n_tensors, self._tiles,
            self._flat[0].data_ptr(), self._flat[1].data_ptr(), _lib.stream_ptr(self.device)), self.symbols, check_pointers)
        if self._tiles > 0:
            _lib.mark_written(list(self._flat))
        return out
