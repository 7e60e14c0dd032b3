"""Torch-owned device buffers for the tests that call the C ABI directly
(test_gpu_*_abi.py): arrays of any element type go up as bytes, optionally
one element into a larger buffer so the pointer is element-aligned only."""
import numpy as np


class Dev:
    def __init__(self):
        import torch
        import openr_amd.capi as capi
        self.torch, self.capi, self.lib = torch, capi, capi.load()
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)

    def put(self, a, offset=0):
        """a on the device, `offset` elements into a 16-byte aligned buffer"""
        a = np.ascontiguousarray(a)
        raw = a.view(np.uint8).reshape(-1)
        skip = offset * a.dtype.itemsize
        buf = self.torch.empty(raw.size + skip + 16, dtype=self.torch.uint8, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[skip:skip + raw.size]
        view.copy_(self.torch.from_numpy(raw))
        return view

    def get(self, t, dtype=np.uint32):
        return t.cpu().numpy().view(dtype)

    def sync(self):
        self.torch.cuda.synchronize()


def ptr(t):
    return None if t is None else t.data_ptr()
