# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""GPU buffers with poisoned surroundings, shared by the op-level GPU
tests (test_decode_kernels_gpu.py, test_attn_mfma_gpu.py)."""

import torch

PAD = 64        # fence elements on either side: keeps 16-byte alignment


class Fenced:
    """`values` (or NaN of that shape and dtype) on the GPU inside a
    flat buffer that is NaN (0x7F) everywhere else: PAD elements on both
    sides, and `spare` elements of NaN capacity behind the values that
    belong to `.all` but not to `.t`."""

    def __init__(self, values=None, shape=None, dtype=None, spare=0):
        if values is None:
            values = torch.full(shape, self.poison(dtype), dtype=dtype)
        n = values.numel()
        flat = torch.full((PAD + n + spare + PAD,),
                          self.poison(values.dtype), dtype=values.dtype)
        flat[PAD:PAD + n] = values.reshape(-1)
        self.buf = flat.cuda()
        self.n, self.spare = n, spare
        self.t = self.buf[PAD:PAD + n].view(values.shape)
        self.all = self.buf[PAD:PAD + n + spare]
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    @staticmethod
    def poison(dtype):
        return 0x7F if dtype == torch.uint8 else float("nan")

    def intact(self):
        """Nothing wrote outside the values."""
        outside = torch.cat([self.buf[:PAD], self.buf[PAD + self.n:]])
        if outside.dtype == torch.uint8:
            return bool((outside == 0x7F).all())
        return bool(torch.isnan(outside).all())
