"""ctypes binding of libmdx_hip.so (include/mdx.h).  No torch types cross this boundary: tensors are
handed over as raw device pointers + sizes, the current HIP stream as a void*.

The binding is read from the header alone: its prototypes give every entry point's argtypes / restype, its #defines the
constants below.  Call through `api` (checked); `lib()` is the typed raw handle, for callers that want a status code.

There is NO fallback: if the library is missing or a tensor is not a contiguous float32 CUDA/HIP
tensor, the call raises.
"""
import ctypes as C
import os
import re

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MDX_LIB") or os.path.join(_PKG, "libmdx_hip.so")   # MDX_LIB: developer override (kernel A/B builds)
HEADER = os.path.join(os.path.dirname(_PKG), "include", "mdx.h")
_lib = None


class MdxError(RuntimeError):
    pass


with open(HEADER) as _f:
    _HEADER_TEXT = _f.read()
DEFINES = {k: int(v) for k, v in re.findall(r"^#define\s+MDX_(\w+)\s+(\d+)u?\b", _HEADER_TEXT, re.M)}
MAX_SRC, MAX_SCALES, FLAG_AUTOMASK = DEFINES["MAX_SRC"], DEFINES["MAX_SCALES"], DEFINES["FLAG_AUTOMASK"]

# C types of the prototypes -> ctypes.  Every pointer parameter is a c_void_p: it takes ptr()'s c_void_p, C.byref(struct),
# ctypes arrays, None and plain integers.
_ARGTYPES = {"int": C.c_int, "size_t": C.c_size_t, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_RESTYPES = {"int": C.c_int, "size_t": C.c_size_t, "void": None, "void *": C.c_void_p, "const char *": C.c_char_p}


def _ctype(table, decl, entry):
    t = " ".join(decl.replace("*", " * ").split())
    if table is _ARGTYPES and "*" in t:
        return C.c_void_p
    if t not in table:
        raise MdxError("include/mdx.h: %s has a parameter or result of type '%s', which the binding does not map" % (entry, t))
    return table[t]


def signatures():
    """{entry point: (restype, [argtypes])} for every prototype of include/mdx.h."""
    code = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", _HEADER_TEXT, flags=re.S), flags=re.M)
    sigs = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(mdx_\w+)\s*\(([^()]*)\)\s*;", code):
        params = [] if params.strip() == "void" else [re.sub(r"\w+\s*$", "", p) for p in params.split(",")]
        sigs[name] = (_ctype(_RESTYPES, ret, name), [_ctype(_ARGTYPES, p, name) for p in params])
    return sigs


class Desc(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("S", C.c_int32), ("flags", C.c_uint32), ("disp_a", C.c_float), ("disp_b", C.c_float)]


class Sources(C.Structure):
    _fields_ = [("img", C.c_void_p * MAX_SRC)]


class TrainDesc(C.Structure):   # mdx_train_desc
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("S", C.c_int32), ("nscales", C.c_int32),
                ("flags", C.c_uint32), ("disp_a", C.c_float), ("disp_b", C.c_float),
                ("h", C.c_int32 * MAX_SCALES), ("w", C.c_int32 * MAX_SCALES), ("rows_per_chunk", C.c_int32)]


class Timing(C.Structure):   # mdx_timing: hipEvent_t pair recorded right before / after the fused kernel
    _fields_ = [("start", C.c_void_p), ("stop", C.c_void_p)]


class _Api(object):
    """api.mdx_x(...): the entry points of include/mdx.h, checked.  A call with more or fewer arguments than the prototype
    raises TypeError before anything runs (ctypes itself only refuses too few); an int-returning entry point that returns
    a negative status raises MdxError; anything else returns the result."""

    def __getattr__(self, name):
        fn = getattr(lib(), name) if name.startswith("mdx_") else None
        if fn is None or fn.argtypes is None:
            raise AttributeError("include/mdx.h declares no %s" % name)
        nargs, status = len(fn.argtypes), fn.restype is C.c_int

        def call(*args):
            if len(args) != nargs:
                raise TypeError("%s takes %d arguments (include/mdx.h), %d given" % (name, nargs, len(args)))
            r = fn(*args)
            if status and r < 0:
                check(r, name)
            return r
        call.__name__ = name
        setattr(self, name, call)
        return call


api = _Api()


def lib():
    """The typed raw handle of libmdx_hip.so; raises MdxError loudly if it is absent, incomplete or not built from this
    include/mdx.h."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) and not os.environ.get("MDX_LIB"):
            # source-only checkout on a machine with the ROCm toolchain: compile the kernels now (this is the
            # product path building itself, not a fallback -- without hipcc the error below stands)
            try:
                import importlib.util
                spec = importlib.util.spec_from_file_location(
                    "_mdx_build", os.path.join(os.path.dirname(LIB_PATH), "build.py"))
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                mod.build()
            except Exception as exc:  # noqa: BLE001
                raise MdxError("libmdx_hip.so is missing and could not be built with hipcc: %s" % exc)
        if not os.path.exists(LIB_PATH):
            raise MdxError("libmdx_hip.so not found at %s -- build it with "
                           "`python __graft_entry__.py build` (hipcc --offload-arch=gfx950); "
                           "there is no CPU/eager fallback" % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in signatures().items():
            try:
                fn = getattr(handle, name)
            except AttributeError:
                raise MdxError("libmdx_hip.so does not export %s (stale build?)" % name)
            fn.restype, fn.argtypes = res, args
        if handle.mdx_version() != DEFINES["VERSION"]:
            raise MdxError("libmdx_hip.so is MDX_VERSION %d but include/mdx.h says %d (stale build?)"
                           % (handle.mdx_version(), DEFINES["VERSION"]))
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        raise MdxError("%s failed: %s (%d)" % (what, lib().mdx_status_string(status).decode(), status))


def ptr(t, dtype=torch.float32, optional=False, cl=False):
    """Raw device pointer of a contiguous CUDA/HIP tensor (cl: of a 4-D tensor whose memory is channels-last, [B][H][W][C];
    cl="any": dense in either of the two formats -- the caller hands the strides to the kernel)."""
    if t is None:
        if optional:
            return None
        raise MdxError("required tensor is None")
    if not t.is_cuda:
        raise MdxError("mdx kernels run on the GPU only: got a %s tensor (no CPU fallback)" % t.device)
    if cl == "any":
        if t.dtype != dtype or t.dim() != 4 or not (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)):
            raise MdxError("expected a dense %s 4-D tensor, got %s %s strides %s" % (dtype, t.dtype, tuple(t.shape), t.stride()))
    elif cl:
        if t.dtype != dtype or t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last):
            raise MdxError("expected a channels-last %s map, got %s %s strides %s" % (dtype, t.dtype, tuple(t.shape), t.stride()))
    elif t.dtype != dtype or not t.is_contiguous():
        raise MdxError("expected contiguous %s, got %s contiguous=%s" % (dtype, t.dtype, t.is_contiguous()))
    if t.device.index != torch.cuda.current_device():
        # stream() hands the CURRENT device's stream to the library: kernels would run on that device with another
        # device's pointers (a GPU memory fault, not an error code)
        raise MdxError("tensor lives on %s but the current device is cuda:%d -- call torch.cuda.set_device / "
                       "`with torch.cuda.device(...)` first" % (t.device, torch.cuda.current_device()))
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _capturing():
    """True while the current HIP stream is being captured into a graph."""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def host_tensor(structs, dtype=torch.uint8):
    """The bytes of a ctypes structure or array as a host tensor of its own (a copy)."""
    return torch.frombuffer(bytearray(bytes(structs)), dtype=dtype).clone()


def read_structs(who, buf, struct_type, count):
    """`buf` (a tensor, read on the host: synchronises) as `count` ctypes structures; `who` names the caller in the refusal."""
    if _capturing():
        raise MdxError("%s() synchronises and the current stream is being captured" % who)
    return (struct_type * count).from_buffer_copy(buf.cpu().numpy().tobytes())


def workspace(nbytes, device):
    """A scratch buffer of at least `nbytes` (what an mdx_*_workspace_bytes() returned) for one launch: uint8, so hand it over
    as ptr(ws, torch.uint8).  Whole 16-byte units and never empty; the base is aligned to 16 bytes and more, as every
    allocation of torch's is (512 on the GPU, 64 on the host) -- the training kernel addresses it in 16-byte units."""
    return torch.empty(max((int(nbytes) + 15) & ~15, 16), dtype=torch.uint8, device=device)


def make_desc(B, H, W, h, w, S, automask, min_depth, max_depth):
    d = Desc()
    api.mdx_desc_init(C.byref(d), B, H, W, h, w, S, int(bool(automask)), min_depth, max_depth)
    return d


def make_train_desc(B, H, W, S, hw, automask, min_depth, max_depth, rows_per_chunk=0):
    """hw: [(h_s, w_s)] per scale."""
    if not 1 <= len(hw) <= MAX_SCALES:
        raise MdxError("1..%d scales supported, got %d" % (MAX_SCALES, len(hw)))
    d = TrainDesc()
    hs = (C.c_int32 * len(hw))(*[int(x[0]) for x in hw])
    ws = (C.c_int32 * len(hw))(*[int(x[1]) for x in hw])
    api.mdx_train_desc_init(C.byref(d), B, H, W, S, len(hw), hs, ws, int(bool(automask)), min_depth, max_depth,
                            int(rows_per_chunk))
    return d


def ptr_array(tensors, dtype=torch.float32, optional=False):
    """Host array of device pointers (one per scale); None entries allowed when optional."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        p = ptr(t, dtype, optional=optional)
        arr[i] = p.value if p is not None else None
    return arr


def make_sources(tensors):
    s = Sources()
    if not 1 <= len(tensors) <= MAX_SRC:
        raise MdxError("1..%d source frames supported, got %d" % (MAX_SRC, len(tensors)))
    for i, t in enumerate(tensors):
        s.img[i] = ptr(t).value
    return s
