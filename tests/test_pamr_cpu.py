"""Pixel-adaptive mask refinement without a GPU: the torch restatement tests/pamr_ref.py is pinned to fixtures written by the
reference's own PAMR module (tests/golden/make_pamr_golden.py), and the product side is checked as far as the host goes --
the module imports, the two C entries are declared and refuse bad arguments before touching a device, the host module
refuses CPU tensors, and the list hook is there."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import abi_checks
from conftest import GOLDEN
from pamr_ref import pamr_ref

TAGS = ["a", "b", "c", "d"]


def _fixture(tag):
    g = np.load(os.path.join(GOLDEN, "pamr_%s.npz" % tag))
    return (torch.from_numpy(g["x"]), torch.from_numpy(g["mask"]), int(g["num_iter"]), [int(d) for d in g["dilations"]],
            g["ref32"], g["ref64"])


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from acr_wsss_amd import _lib
    return _lib


def test_fixtures_are_the_stated_cases():
    shapes = {t: _fixture(t) for t in TAGS}
    assert tuple(shapes["a"][0].shape) == (1, 3, 48, 64) and tuple(shapes["a"][1].shape) == (1, 4, 48, 64)
    assert tuple(shapes["b"][0].shape) == (2, 3, 40, 52) and tuple(shapes["b"][1].shape) == (2, 3, 10, 13)
    assert tuple(shapes["c"][0].shape[-2:]) == (20, 30)
    for t in "abc":
        assert shapes[t][2] == 10 and shapes[t][3] == [1, 2, 4, 8, 12, 24]
    assert shapes["d"][2] == 1 and shapes["d"][3] == [1] and shapes["d"][1].shape[1] == 1
    x = shapes["a"][0]
    assert (x[:, :, 6:22, 8:30] == x[:, :, 6:7, 8:9]).all()                 # the exactly flat block
    for t in TAGS:
        assert shapes[t][4].dtype == np.float32 and shapes[t][5].dtype == np.float64


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_reference_in_float64(tag):
    x, mask, num_iter, dil, _, ref64 = _fixture(tag)
    out = pamr_ref(x.double(), mask.double(), num_iter, dil).numpy()
    err = float(np.abs(out - ref64).max())
    print("pamr_%s float64: max|pamr_ref - ref64| = %.3e" % (tag, err))
    assert out.dtype == np.float64 and err <= 1e-12


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_in_float32_within_twice_the_reference_error(tag):
    x, mask, num_iter, dil, ref32, ref64 = _fixture(tag)
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    out = pamr_ref(x, mask, num_iter, dil).numpy()
    err = float(np.abs(out.astype(np.float64) - ref64).max())
    print("pamr_%s float32: E_ref = %.3e, max|pamr_ref - ref64| = %.3e" % (tag, e_ref, err))
    assert out.dtype == np.float32 and 0 < e_ref and err <= 2 * e_ref


def test_restatement_gives_uniform_weights_on_a_flat_image():
    """deviation 0 and every difference 0: a = -0 / 1e-8, the softmax is exactly uniform"""
    from pamr_ref import pamr_weights
    w = pamr_weights(torch.full((1, 3, 9, 11), 0.3), (1, 2))
    assert torch.equal(w, torch.full_like(w, 1.0 / 16))


def test_module_imports_and_signatures_hold_the_entries():
    from acr_wsss_amd import _lib, pamr
    assert {"acr_pamr_affinity", "acr_pamr_propagate"} <= set(_lib.SIGNATURES)
    assert [len(abi_checks.declared(n)[1]) for n in ("acr_pamr_affinity", "acr_pamr_propagate")] == [9, 10]
    assert _lib.SIGNATURES["acr_pamr_affinity"][0] is ctypes.c_int32 and len(_lib.SIGNATURES["acr_pamr_affinity"][1]) == 9
    assert _lib.SIGNATURES["acr_pamr_propagate"][0] is ctypes.c_int32 and len(_lib.SIGNATURES["acr_pamr_propagate"][1]) == 10
    sig = inspect.signature(pamr.pamr)
    assert sig.parameters["num_iter"].default == 1 and tuple(sig.parameters["dilations"].default) == (1,)
    mod = pamr.PAMR()
    assert isinstance(mod, torch.nn.Module) and mod.num_iter == 1 and list(mod.dilations) == [1]
    assert len(list(mod.parameters())) == 0


def test_no_cpu_path(built):
    from acr_wsss_amd.pamr import PAMR, pamr, pamr_with_alpha
    x, m = torch.rand(1, 3, 8, 9), torch.rand(1, 2, 8, 9)
    with pytest.raises(built.AcrHipError):
        pamr(x, m)
    with pytest.raises(built.AcrHipError):
        PAMR(2, [1, 2])(x, m)
    with pytest.raises(built.AcrHipError):
        pamr_with_alpha({3: np.zeros((8, 9), np.float32)}, (1, 12), np.zeros((8, 9, 3), np.uint8), device="cpu")


def test_infer_cam_list_accepts_out_pamr():
    from acr_wsss_amd.infer_cam import infer_cam_list
    p = inspect.signature(infer_cam_list).parameters
    assert p["out_pamr"].default is None and p["pamr_iter"].default == 10
    assert tuple(p["pamr_dilations"].default) == (1, 2, 4, 8, 12, 24)


def test_c_entries_refuse_bad_arguments_on_the_host(built):
    """argument checks come before any launch: negative status and a message, no device touched"""
    lib = built.load()
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below fails its checks first
    null = ctypes.c_void_p(0)

    def dil(*v):
        return (ctypes.c_int32 * len(v))(*v)

    def refused(rc, word):
        msg = lib.acr_last_error().decode()
        assert rc < 0 and word in msg, (rc, msg)

    refused(lib.acr_pamr_affinity(null, 1, 3, 8, 8, dil(1), 1, fake, None), "null")
    refused(lib.acr_pamr_affinity(fake, 1, 3, 8, 8, dil(1), 1, null, None), "null")
    refused(lib.acr_pamr_affinity(fake, 1, 3, 8, 8, None, 1, fake, None), "null")
    refused(lib.acr_pamr_affinity(fake, 1, 3, 8, 8, dil(1), 0, fake, None), "n_dil")
    refused(lib.acr_pamr_affinity(fake, 1, 3, 8, 8, dil(*range(1, 10)), 9, fake, None), "n_dil")
    refused(lib.acr_pamr_affinity(fake, 1, 3, 8, 8, dil(1, 0), 2, fake, None), "dilation")
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, -1, 8), (1, 3, 8, 0)):
        refused(lib.acr_pamr_affinity(fake, *dims, dil(1), 1, fake, None), "geometry")
    other = ctypes.c_void_p(8192)
    refused(lib.acr_pamr_propagate(null, fake, other, 1, 2, 8, 8, dil(1), 1, None), "null")
    refused(lib.acr_pamr_propagate(fake, null, other, 1, 2, 8, 8, dil(1), 1, None), "null")
    refused(lib.acr_pamr_propagate(fake, fake, null, 1, 2, 8, 8, dil(1), 1, None), "null")
    refused(lib.acr_pamr_propagate(fake, other, other, 1, 2, 8, 8, dil(1), 1, None), "different")
    refused(lib.acr_pamr_propagate(fake, fake, other, 1, 2, 8, 8, None, 1, None), "null")
    refused(lib.acr_pamr_propagate(fake, fake, other, 1, 2, 8, 8, dil(1), 9, None), "n_dil")
    refused(lib.acr_pamr_propagate(fake, fake, other, 1, 2, 8, 8, dil(-3), 1, None), "dilation")
    for dims in ((0, 2, 8, 8), (1, 0, 8, 8), (1, 2, 0, 8), (1, 2, 8, -4)):
        refused(lib.acr_pamr_propagate(fake, fake, other, *dims, dil(1), 1, None), "geometry")
