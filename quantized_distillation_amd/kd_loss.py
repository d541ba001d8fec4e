"""The distillation losses of harness.models with value and logit gradient from ONE call of libqd_loss.so (include/qd_loss.h):

    fused_kd_loss(student_logits, teacher_logits, labels, temperature=2.0, teacher_weight=0.7)       # models.kd_loss
    fused_word_kd_loss(student_logits, teacher_logits, target, batch, pad=1, teacher_weight=0.7)     # models.word_kd_loss

Both are differentiable with respect to student_logits alone (the teacher is a constant of distillation) and return a 0-d tensor.
forward makes the one call, which also writes d loss / d student_logits; backward multiplies that by the upstream gradient -- one
extra pass over the gradient, a read and a write, that a loss whose upstream gradient is always 1 would not need.

fp32, 2-D tensors on a HIP device only: TypeError / ValueError for anything else before any launch, NotImplementedError for CPU
tensors -- there is no CPU path and no fallback.
"""
import math

import torch

from . import _lib, _loss


def _validated(student, teacher, target):
    for name, t in (('student_logits', student), ('teacher_logits', teacher), ('target', target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s: a tensor, got %s' % (name, type(t).__name__))
    if student.dtype != torch.float32 or teacher.dtype != torch.float32:
        raise TypeError('student_logits and teacher_logits: float32, got %s and %s' % (student.dtype, teacher.dtype))
    if target.dtype != torch.int64:
        raise TypeError('target: int64, got %s' % target.dtype)
    if student.dim() != 2 or student.shape[1] == 0:
        raise ValueError('student_logits: [rows, cols] with cols > 0, got %s' % (tuple(student.shape),))
    if teacher.shape != student.shape or tuple(target.shape) != (student.shape[0],):
        raise ValueError('teacher_logits %s and target %s do not fit student_logits %s'
                         % (tuple(teacher.shape), tuple(target.shape), tuple(student.shape)))
    if student.device.type != 'cuda' or teacher.device != student.device or target.device != student.device:
        if student.device.type == 'cpu':
            raise NotImplementedError('HIP device only')
        raise ValueError('student_logits, teacher_logits and target: one HIP device, got %s, %s and %s'
                         % (student.device, teacher.device, target.device))


def _temperature(temperature):
    if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
        raise ValueError('temperature: a finite number > 0, got %r' % (temperature,))
    return float(temperature)


def kd_loss_rows(student, teacher, target, temperature, kl_scale, nll_scale, ignore_index):
    """The call itself: (loss [1], grad [rows, cols], row_kl [rows], row_nll [rows]) of qdl_kd_loss_f32 on torch's current stream."""
    _validated(student, teacher, target)
    temperature = _temperature(temperature)
    z, t, y = student.detach().contiguous(), teacher.detach().contiguous(), target.contiguous()
    rows, cols = z.shape
    grad = torch.empty_like(z)
    row_kl, row_nll = torch.empty(rows, dtype=torch.float32, device=z.device), torch.empty(rows, dtype=torch.float32, device=z.device)
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        _loss.check(_loss.load().qdl_kd_loss_f32(z.data_ptr(), t.data_ptr(), y.data_ptr(), rows, cols, temperature, kl_scale, nll_scale, ignore_index,
                                                  grad.data_ptr(), row_kl.data_ptr(), row_nll.data_ptr(), loss.data_ptr(), _lib.stream_ptr(z.device)))
    return loss, grad, row_kl, row_nll


class _FusedKd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, target, temperature, kl_scale, nll_scale, ignore_index):
        loss, grad, _, _ = kd_loss_rows(student, teacher, target, temperature, kl_scale, nll_scale, ignore_index)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad * grad_output, None, None, None, None, None, None


def _weight(teacher_weight):
    if not isinstance(teacher_weight, (int, float)):
        raise TypeError('teacher_weight: a number, got %s' % type(teacher_weight).__name__)
    return float(teacher_weight)


def fused_kd_loss(student_logits, teacher_logits, labels, temperature=2.0, teacher_weight=0.7):
    """models.kd_loss: teacher_weight T^2 KLDiv(log_softmax(zs / T), softmax(zt / T)) with the ELEMENT-mean reduction, plus
    (1 - teacher_weight) cross entropy with the batch-mean reduction.  No label is ignored."""
    w, temperature = _weight(teacher_weight), _temperature(temperature)
    _validated(student_logits, teacher_logits, labels)
    if student_logits.shape[0] == 0:
        raise ValueError('student_logits: at least one row (the mean over no rows is not defined)')
    rows, cols = student_logits.shape
    no_index = -1 - (1 << 62)                                            # ignore_index: a value no label has; a negative label is out of range, loud
    return _FusedKd.apply(student_logits, teacher_logits, labels, temperature, w * temperature ** 2 / (rows * cols), (1.0 - w) / rows, no_index)


def fused_word_kd_loss(student_logits, teacher_logits, target, batch, pad=1, teacher_weight=0.7):
    """models.word_kd_loss: (1 - teacher_weight) NLL + teacher_weight KL(teacher || student) at T = 1, the positions whose target
    is `pad` left out (not even read), summed over the tokens and divided by `batch`."""
    w = _weight(teacher_weight)
    if not isinstance(batch, int) or isinstance(batch, bool) or batch < 1:
        raise ValueError('batch: a positive int, got %r' % (batch,))
    if not isinstance(pad, int) or isinstance(pad, bool):
        raise TypeError('pad: an int, got %s' % type(pad).__name__)
    return _FusedKd.apply(student_logits, teacher_logits, target, 1.0, w / batch, (1.0 - w) / batch, pad)
