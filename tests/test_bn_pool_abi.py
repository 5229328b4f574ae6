"""CPU: the fused stem entry point of csrc/norm_nhwc.hip (mdx_bn_pool_nhwc_fwd: relu(bn(x)) -> max-pool 3x3/2/1 as one operator)
and the A/B switch mdx_bn_dz_once -- prototypes parsed and exported, and what the entry point refuses, with which status and in
which order (NULL pointer, bad shape, misaligned, workspace: the order of its mdx_bn_act_nhwc_* siblings).
Every case returns before the first launch: the pointers are dummy addresses and no GPU is needed."""
import ctypes as C
import importlib

import pytest

PKG = "digging-into-self-supervised-monocular-depth-estimation_amd"
importlib.import_module(PKG)
from mdx import _lib  # noqa: E402

OK_SHAPE, NULL, WS, ALIGN = -1, -2, -3, -6     # MDX_ERR_BAD_SHAPE, _NULL_POINTER, _WORKSPACE, _MISALIGNED
P = 4096                                       # non-null, 16-byte aligned, never dereferenced on these paths
ODD = P + 4                                    # 4-byte but not 8- or 16-byte aligned
BN = dict(B=2, C=8, H=4, W=6)

# entry point -> its parameters in prototype order with values that pass every check (a call with only these would launch)
ENTRIES = {
    "mdx_bn_pool_nhwc_fwd": dict(x=P, gamma=P, beta=P, run_mean=P, run_var=P, y=None, pooled=P, arg=P, save_mean=P, save_invstd=P,
                                 **BN, groups=1, eps=1e-5, momentum=0.1, dtype=0, workspace=P, workspace_bytes=128, stream=None),
}
REQUIRED = {
    "mdx_bn_pool_nhwc_fwd": "x gamma beta pooled arg save_mean save_invstd workspace run_mean run_var",   # running statistics: both or none
}
ALIGNED = {      # every map pointer, the optional ones included
    "mdx_bn_pool_nhwc_fwd": "x y pooled arg",
}


def _call(name, **over):
    args = dict(ENTRIES[name])
    unknown = set(over) - set(args)
    assert not unknown, (name, unknown)
    args.update(over)
    fn = getattr(_lib.lib(), name)
    assert len(fn.argtypes) == len(args), name
    return fn(*args.values())


def test_prototypes_are_parsed_and_exported():
    sigs = _lib.signatures()
    lib = _lib.lib()
    for name, args in ENTRIES.items():
        res, argtypes = sigs[name]
        assert res is C.c_int and len(argtypes) == len(args), name
        for (arg, value), ctype in zip(args.items(), argtypes):
            assert (ctype is C.c_void_p) == (value is None or value == P), (name, arg)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == argtypes, name
    assert sigs["mdx_bn_dz_once"] == (C.c_int, [C.c_int]) and hasattr(lib, "mdx_bn_dz_once")
    assert lib.mdx_version() == 510


def test_the_workspace_is_the_batch_norm_one():
    assert _lib.lib().mdx_bn_nhwc_workspace_bytes(2, 8, 4, 6, 1, 0) == 128
    for name in ENTRIES:
        assert _call(name, workspace_bytes=0) == WS


@pytest.mark.parametrize("name,arg", [(n, a) for n, v in REQUIRED.items() for a in v.split()])
def test_each_required_pointer_null(name, arg):
    assert _call(name, **{arg: None}) == NULL


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("over", [dict(dtype=2), dict(dtype=-1), dict(dtype=1),       # bfloat16 keeps the two-operator path
                                  dict(C=6), dict(C=0), dict(B=0), dict(H=-1), dict(W=0), dict(groups=0), dict(groups=65536),
                                  dict(B=65536, H=32768)])
def test_bad_dtype_and_shape(name, over):
    assert _call(name, **over) == OK_SHAPE


@pytest.mark.parametrize("name,arg", [(n, a) for n, v in ALIGNED.items() for a in v.split()])
def test_pointer_misaligned_by_four_bytes(name, arg):
    assert _call(name, **{arg: ODD}) == ALIGN


@pytest.mark.parametrize("name", list(ENTRIES))
def test_workspace_one_byte_too_small(name):
    assert _call(name, workspace_bytes=ENTRIES[name]["workspace_bytes"] - 1) == WS
    assert _call(name, B=4, workspace_bytes=_lib.lib().mdx_bn_nhwc_workspace_bytes(4, 8, 4, 6, 1, 0) - 1) == WS


@pytest.mark.parametrize("name, over, status", [
    # two rules at once: NULL wins over shape, shape over alignment, alignment over the workspace
    ("mdx_bn_pool_nhwc_fwd", dict(pooled=None, C=6), NULL),
    ("mdx_bn_pool_nhwc_fwd", dict(run_var=None, dtype=2), NULL),
    ("mdx_bn_pool_nhwc_fwd", dict(C=6, x=ODD), OK_SHAPE),
    ("mdx_bn_pool_nhwc_fwd", dict(y=ODD, workspace_bytes=0), ALIGN),
    ("mdx_bn_pool_nhwc_fwd", dict(arg=None, dtype=1), NULL),
    ("mdx_bn_pool_nhwc_fwd", dict(dtype=1, pooled=ODD), OK_SHAPE),
    ("mdx_bn_pool_nhwc_fwd", dict(arg=ODD, workspace_bytes=127), ALIGN),
])
def test_which_check_wins(name, over, status):
    assert _call(name, **over) == status


def test_dz_once_switch_returns_the_previous_setting():
    lib = _lib.lib()
    was = lib.mdx_bn_dz_once(0)
    try:
        assert lib.mdx_bn_dz_once(1) == 0 and lib.mdx_bn_dz_once(5) == 1 and lib.mdx_bn_dz_once(1) == 1
    finally:
        lib.mdx_bn_dz_once(was)
