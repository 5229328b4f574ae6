"""CPU: the eval-mode batch-norm entry points (csrc/norm_infer.hip) -- declared by include/mdx.h with the documented
prototypes, exported by the built library, and refusing bad arguments with status codes before any HIP call (no kernel
is launched, no GPU needed)."""
import ctypes as C
import importlib
import os
import re

import pytest

PKG = "digging-into-self-supervised-monocular-depth-estimation_amd"
importlib.import_module(PKG)
from mdx import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mdx_bn_act_infer", "mdx_bn_act_nhwc_infer")
# x, res, gamma, beta, run_mean, run_var, y, B, C, H, W, eps, relu, dtype, stream
PROTO = [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_int, C.c_void_p]
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address that is never dereferenced on these paths


@pytest.mark.parametrize("name", ENTRIES)
def test_header_declares_the_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert _lib.signatures()[name] == (C.c_int, PROTO)


@pytest.mark.parametrize("name", ENTRIES)
def test_built_library_exports_the_entry(name):
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, name)
    fn = getattr(_lib.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == PROTO


def _call(name, x=FAKE, res=None, gamma=FAKE, beta=FAKE, mean=FAKE, var=FAKE, y=FAKE, B=2, Cc=64, H=4, W=6, dtype=0):
    return getattr(_lib.lib(), name)(x, res, gamma, beta, mean, var, y, B, Cc, H, W, 1e-5, 1, dtype, None)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("missing", ["x", "gamma", "beta", "mean", "var", "y"])
def test_null_pointers_are_refused(name, missing):
    assert _call(name, **{missing: None}) == -2          # MDX_ERR_NULL_POINTER


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("size", ["B", "Cc", "H", "W"])
@pytest.mark.parametrize("value", [0, -3])
def test_non_positive_sizes_are_refused(name, size, value):
    assert _call(name, **{size: value}) == -1            # MDX_ERR_BAD_SHAPE


@pytest.mark.parametrize("name", ENTRIES)
def test_unknown_dtype_is_refused(name):
    assert _call(name, dtype=2) == -1


def test_channels_last_needs_whole_channel_vectors():
    """A thread of the channels-last kernel owns one 16-byte channel vector: 4 float32 / 8 bfloat16 channels."""
    for Cc, dtype in ((6, 0), (2, 0), (12, 1), (4, 1)):
        assert _call("mdx_bn_act_nhwc_infer", Cc=Cc, dtype=dtype) == -1, (Cc, dtype)
    # the planar entry point takes any channel count: its argument checks pass these (then it would launch, so not called here)


def test_misaligned_pointers_are_refused():
    odd = C.c_void_p(4096 + 8)                           # 8-byte but not 16-byte aligned
    assert _call("mdx_bn_act_nhwc_infer", x=odd) == -6   # MDX_ERR_MISALIGNED
    assert _call("mdx_bn_act_nhwc_infer", y=odd) == -6
    assert _call("mdx_bn_act_nhwc_infer", res=odd) == -6
    assert _call("mdx_bn_act_infer", x=C.c_void_p(4096 + 2)) == -6            # float32 maps: element-aligned
    assert _call("mdx_bn_act_infer", res=C.c_void_p(4096 + 1), dtype=1) == -6   # bfloat16: 2-byte aligned


def test_python_entry_has_no_cpu_fallback():
    import torch
    from mdx import functional as F
    x = torch.zeros(1, 4, 2, 2)
    p = torch.ones(4)
    with pytest.raises(_lib.MdxError, match="GPU|CUDA"):
        F.bn_act_infer(x, p, p, p, p)


def test_eval_batch_norm_on_the_cpu_takes_the_torch_ops():
    """BatchNorm2d.act in eval mode on a CPU tensor: the module's own batch norm (+ residual, ReLU); nothing is counted."""
    import torch
    from model_layer.depth_encoder import BatchNorm2d
    torch.manual_seed(0)
    bn = BatchNorm2d(8).eval()
    with torch.no_grad():
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    x, r = torch.randn(2, 8, 3, 5), torch.randn(2, 8, 3, 5)
    with torch.no_grad():
        y = bn.act(x, residual=r)
        want = torch.relu(torch.nn.functional.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False,
                                                         0.1, bn.eps) + r)
    assert torch.equal(y, want)
    assert bn._pending_batches == 0 and int(bn.num_batches_tracked) == 0
