"""`freqencoder` operator API on MI355X (reference: freqencoder/freq.py:15-77)."""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

from .. import _lib


class _freq_encoder(Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)  # float32 also under autocast, as the reference (freq.py:17)
    def forward(ctx, inputs, degree, output_dim):
        """inputs [B, input_dim] float -> [B, output_dim] float32, output_dim = input_dim (1 + 2 degree)  (freq.py:18-34)"""
        inputs = inputs.contiguous()
        B, input_dim = inputs.shape
        if output_dim != input_dim + 2 * input_dim * degree:
            raise ValueError(f"freq_encode: output_dim {output_dim} is not input_dim (1 + 2 degree) = {input_dim + 2 * input_dim * degree}")
        outputs = torch.empty(B, output_dim, dtype=inputs.dtype, device=inputs.device)
        _lib.call("freq_encode_forward", inputs, outputs, B, input_dim, degree)
        # the inputs alone: the backward recomputes sin / cos from them (the reference keeps the [B, output_dim] outputs, freq.py:31)
        ctx.save_for_backward(inputs)
        ctx.dims = [B, input_dim, degree]
        return outputs

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        grad = grad.contiguous().float()
        (inputs,) = ctx.saved_tensors
        B, input_dim, degree = ctx.dims
        grad_inputs = torch.empty_like(inputs)  # written, not accumulated
        _lib.call("freq_encode_backward", grad, inputs, B, input_dim, degree, grad_inputs)
        return grad_inputs, None, None


freq_encode = _freq_encoder.apply


class FreqEncoder(nn.Module):
    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = input_dim + input_dim * 2 * degree
        assert self.input_dim >= 1, "frequency encoder needs input dim >= 1"
        assert 0 <= self.degree <= 16, "frequency encoder only supports degree in [0, 16]"

    def __repr__(self):
        return f"FreqEncoder: input_dim={self.input_dim} degree={self.degree} output_dim={self.output_dim}"

    def forward(self, inputs, **kwargs):
        """inputs [..., input_dim] -> [..., output_dim]; `bound` / `size` are accepted and ignored (the reference does not normalise)"""
        prefix_shape = list(inputs.shape[:-1])
        inputs = inputs.reshape(-1, self.input_dim)
        outputs = freq_encode(inputs, self.degree, self.output_dim)
        return outputs.reshape(prefix_shape + [self.output_dim])
