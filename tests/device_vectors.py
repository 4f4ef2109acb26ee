"""Device vectors for the _dev entry points: what the tests hand to them by address.

torch is imported HERE, once, and before the library is loaded.  A torch wheel carries its own HIP runtime and asks for it by a name
that an already loaded libamdhip64.so.N does not answer to: a process that loaded libadflow_gpu.so first gets a second runtime with
torch, torch finds no GPU, and the two abort at exit.  With torch first both share torch's runtime, as in bench.py and tools/ -- so a
-m gpu session that collects a module importing this one runs all its tests on that runtime.  Every check module with a _dev twin
imports this module at its top, i.e. at collection, before the engine fixture loads the library; anything that loads the library at
import ahead of it is refused below, not left to abort."""
import sys

import numpy as np

if "torch" not in sys.modules:
    with open("/proc/self/maps") as _maps:
        if "libamdhip64" in _maps.read():
            raise ImportError("device_vectors: a HIP runtime is already loaded in this process; import device_vectors (torch) before "
                              "anything loads libadflow_gpu.so")
import torch  # noqa: E402

class HostVectors:
    """'device' vectors of the kernel-logic emulator: its hipMalloc is malloc, so a numpy array is a device vector there"""

    def put(self, a):
        return np.array(a, dtype=np.float64, order="C", copy=True)

    def empty(self, n):
        return np.zeros(int(n))

    def ptr(self, v):
        return v.ctypes.data

    def get(self, v):
        return v.copy()

    def sync(self):
        pass

    def pinned(self, a):
        """a caller's host array: here a plain copy (the emulator's copies are synchronous)"""
        return np.array(a, order="F" if a.ndim > 1 and a.flags["F_CONTIGUOUS"] else "C", copy=True)


class TorchVectors:
    """torch float64 tensors on the GPU, handed over by data_ptr(); torch's stream is not the library's: sync() around every call"""

    torch = torch

    def put(self, a):
        return self.torch.from_numpy(np.array(a, dtype=np.float64, order="C", copy=True)).to("cuda")

    def empty(self, n):
        return self.torch.zeros(int(n), dtype=self.torch.float64, device="cuda")

    def ptr(self, v):
        return v.data_ptr()

    def get(self, v):
        self.sync()
        return v.cpu().numpy()

    def sync(self):
        self.torch.cuda.synchronize()

    def pinned(self, a):
        """a caller's host array in page-locked memory (a copy of `a` with its shape and order, viewed through numpy): a
        hipMemcpyAsync from it is truly asynchronous"""
        fortran = a.ndim > 1 and a.flags["F_CONTIGUOUS"]
        flat = self.torch.from_numpy(np.array(a.reshape(-1, order="F" if fortran else "C"), copy=True)).pin_memory()
        assert flat.is_pinned()
        return flat.numpy().reshape(a.shape, order="F" if fortran else "C")


def device_vectors(config):
    """what a -m gpu test hands to a _dev entry point: torch tensors, or numpy arrays when the suite runs with --hostsim (a torch
    pointer means nothing to the emulator)"""
    return HostVectors() if config.getoption("--hostsim") else TorchVectors()


def dev_call(engine, dv, fn, *args, **kw):
    """fn(*args) on device vectors: everything torch enqueued is done before the library starts, and the library is done before
    the result is read"""
    dv.sync()
    out = fn(*args, **kw)
    engine.sync()
    return out
