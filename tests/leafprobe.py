"""TEST INFRASTRUCTURE: the GPU probe of the field leaves (tests/leafprobe/bn254_leafprobe.hip - one kernel per leaf of leaf_list.hpp, one case
per lane, raw limbs in and out) as Python calls, for tests/test_gpu_leaf.py.  The one source is compiled into two objects of one library: with
BN_INLINE_ALL (context "inl": the forced-inline form of the pairing kernels) and without (context "fn": the leaves as real functions).  Needs
torch (device memory) - like the test that uses it.  Never loaded by the product."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "leafprobe" / "bn254_leafprobe.hip"
LIST = HERE / "leafprobe" / "leaf_list.hpp"
LIB = HERE / "leafprobe" / "libbn254_leafprobe.so"
CSRC = HERE.parent / "bn_amd" / "csrc"
CONTEXTS = ("inl", "fn")


def build(force=False):
    """hipcc cross-compiles for gfx950 without a GPU; the .so stays in-tree and travels to the GPU box (__graft_entry__.build calls this).
    The flags are the product's (bn_amd/_native.py); the two objects go through a temporary directory, only the library is kept."""
    import tempfile
    from bn_amd import _native
    deps = [SRC, LIST] + sorted(CSRC.glob("*.hpp"))
    if force or not LIB.exists() or LIB.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        flags = [_native.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"] + _native.DEVICE_FLAGS + [f"-I{CSRC}"]
        with tempfile.TemporaryDirectory() as tmp:
            objs = [str(pathlib.Path(tmp) / "leafprobe_inl.o"), str(pathlib.Path(tmp) / "leafprobe_fn.o")]
            procs = [subprocess.Popen(flags + ["-DBN_INLINE_ALL", "-c", str(SRC), "-o", objs[0]]), subprocess.Popen(flags + ["-c", str(SRC), "-o", objs[1]])]
            if any([p.wait() for p in procs]):
                raise RuntimeError("hipcc failed on " + str(SRC))
            subprocess.check_call(flags + ["-shared"] + objs + ["-o", str(LIB)])
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        from bn_amd import _native
        _native.lib()                                   # binds the process to ONE HIP runtime first (bn_amd/_native.py _preload_shared_hip_runtime)
        if not LIB.exists():
            raise RuntimeError(f"{LIB} is missing: python -c 'import __graft_entry__ as g; g.build()'")
        l = C.CDLL(str(LIB))
        vp = C.c_void_p
        for ctx in CONTEXTS:
            getattr(l, f"bnlp_{ctx}_run").argtypes = [C.c_int, vp, vp, vp, C.c_size_t, vp]; getattr(l, f"bnlp_{ctx}_run").restype = C.c_int
            getattr(l, f"bnlp_{ctx}_leaf_count").restype = C.c_int
            getattr(l, f"bnlp_{ctx}_leaf_info").argtypes = [C.c_int]; getattr(l, f"bnlp_{ctx}_leaf_info").restype = C.c_char_p
        _lib = l
    return _lib


def leaf_table(ctx):
    """[(name, kinds, output limbs)] as compiled into the library"""
    l = lib()
    out = []
    for i in range(getattr(l, f"bnlp_{ctx}_leaf_count")()):
        name, kinds, outw = getattr(l, f"bnlp_{ctx}_leaf_info")(i).decode().split(":")
        out.append((name, kinds, int(outw)))
    return out


def run(ctx, leaf_id, ops, flags, outw, device=0):
    """ONE launch over all cases of a leaf.  ops: uint32 [n, stride], flags: int32 [n].  Returns (result uint32 [n, outw], the operands and
    the flags as read back from the device after the kernel)."""
    import torch
    l = lib()
    dev = torch.device("cuda", device)
    ops = np.array(ops, np.uint32, order="C"); flags = np.array(flags, np.int32, order="C")            # (copies: torch wants writable arrays)
    n = ops.shape[0]
    assert flags.shape == (n,)
    with torch.cuda.device(dev):
        d_ops = torch.from_numpy(ops.view(np.int32)).to(dev)
        d_flags = torch.from_numpy(flags).to(dev)
        d_out = torch.full((n, outw), -1, dtype=torch.int32, device=dev)
        rc = getattr(l, f"bnlp_{ctx}_run")(int(leaf_id), d_ops.data_ptr(), d_flags.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream(dev).cuda_stream)
        if rc:
            raise RuntimeError(f"leaf probe: error {rc}")
        torch.cuda.synchronize(dev)
        return d_out.cpu().numpy().view(np.uint32), d_ops.cpu().numpy().view(np.uint32), d_flags.cpu().numpy()
