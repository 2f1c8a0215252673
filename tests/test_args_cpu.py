"""acr_wsss_amd/_args.py and _lib.workspace on the host: what can be judged without a device is a ValueError that names the
argument, a well-formed host tensor is the AcrHipError of "no CPU path", and a workspace query's refusal carries the library's
own message before anything is allocated."""
import numpy as np
import pytest
import torch

from acr_wsss_amd import _args as A
from acr_wsss_amd import _lib as L

GOOD = torch.zeros(2, 3, 4)
# (x, keywords, a word of the message): each row is wrong in exactly one way, and no row needs a device to be found wrong
BAD = [
    ([[0.0]], {}, "torch tensor"),                                                   # type: not a tensor, no upload asked for
    (np.zeros((2, 3, 4), np.float32), {}, "torch tensor"),                           # type: numpy without upload
    (np.zeros((2, 3, 4), np.float64), dict(upload=True), "float32"),                 # dtype of an array to upload
    (np.zeros((2, 3, 4), np.bool_), dict(upload=True), "float32"),                   # bool counts as uint8 only where asked for
    (GOOD.double(), {}, "float32"),                                                  # dtype
    (GOOD.bool(), {}, "float32"),
    (GOOD[0], dict(shape=(2, "W", "H")), "(2, W, H)"),                               # rank
    (GOOD, dict(shape=("B", "K", "h", "w")), "(B, K, h, w)"),
    (GOOD, dict(shape=(3, "W", "H")), "(3, W, H)"),                                  # shape: a fixed axis
    (GOOD, dict(shape=(2, 3, 5)), "(2, 3, 5)"),
    (np.zeros((2, 3), np.float32), dict(shape=(2, 4), upload=True), "(2, 4)"),       # shape of an array to upload
    (GOOD[:0], {}, "non-empty"),                                                     # emptiness, with and without a shape
    (GOOD[:, :0], dict(shape=(2, "W", "H")), "non-empty"),
    (GOOD.transpose(1, 2), {}, "contiguous"),                                        # contiguity
    (GOOD[:, :, ::2], dict(shape=(2, 3, 2)), "strides"),
]


@pytest.mark.parametrize("row", range(len(BAD)))
def test_tensor_arg_refuses_on_the_host_and_names_the_argument(row):
    x, kw, word = BAD[row]
    for dev in (None, torch.device("cuda", 0)):             # with or without a device to compare with: it is never asked for
        with pytest.raises(ValueError) as e:
            A.tensor_arg(x, "arg_%d" % row, torch.float32, device=dev, **kw)
        assert ("arg_%d" % row) in str(e.value) and word in str(e.value), str(e.value)


def test_tensor_arg_order_of_judgement():
    """dtype before shape before contiguity, all before the device: an input wrong in several ways reports the earliest"""
    x = torch.zeros(3, 4, dtype=torch.float64).t()
    with pytest.raises(ValueError, match="float32 tensor, got torch.float64"):
        A.tensor_arg(x, "x", torch.float32, shape=(5, 5))
    with pytest.raises(ValueError, match=r"non-empty \(5, 5\)"):
        A.tensor_arg(x.float(), "x", torch.float32, shape=(5, 5))
    with pytest.raises(ValueError, match="strides"):
        A.tensor_arg(x.float(), "x", torch.float32, shape=(4, 3))


def test_a_good_host_tensor_has_no_cpu_path():
    for kw in ({}, dict(shape=(2, "W", "H")), dict(device=torch.device("cuda", 0))):
        with pytest.raises(L.AcrHipError, match="no CPU path"):
            A.tensor_arg(GOOD, "x", torch.float32, **kw)
    with pytest.raises(L.AcrHipError):                       # uploaded "to" the host: still no GPU tensor
        A.tensor_arg(GOOD.numpy(), "x", torch.float32, device=torch.device("cpu"), upload=True)
    with pytest.raises(L.AcrHipError):
        A.on_device(GOOD, "x")
    # on_gpu=False: judged, returned, and the device left to the caller
    assert A.tensor_arg(GOOD, "x", torch.float32, shape=(2, 3, 4), on_gpu=False) is GOOD
    assert A.tensor_arg(GOOD.transpose(1, 2), "x", torch.float32, contiguous=False, on_gpu=False).shape == (2, 4, 3)
    up = A.tensor_arg(np.ones((2, 2), np.bool_), "m", torch.uint8, upload=True, bool_as_u8=True, on_gpu=False)
    assert up.dtype == torch.uint8 and up.tolist() == [[1, 1], [1, 1]]
    assert A.tensor_arg(torch.ones(2, 2, dtype=torch.bool), "m", torch.uint8, bool_as_u8=True, on_gpu=False).dtype == torch.uint8


def test_gpu_device(monkeypatch):
    for device in ("cpu", torch.device("cpu")):
        with pytest.raises(L.AcrHipError, match="the stage needs a GPU"):
            A.gpu_device(device, "the stage")
    with pytest.raises(L.AcrHipError):
        A.first_device((None, np.zeros(2), GOOD), "cuda", "the stage")        # the first tensor decides, and it is on the host
    with pytest.raises(L.AcrHipError):
        A.first_device((np.zeros(2),), "cpu", "the stage")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(L.AcrHipError, match="no CPU path"):
        A.gpu_device("cuda", "the stage")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    assert A.gpu_device("cuda", "the stage") == torch.device("cuda", 3)
    assert A.gpu_device("cuda:1", "the stage") == torch.device("cuda", 1)
    assert A.first_device((np.zeros(2),), torch.device("cuda", 2), "the stage") == torch.device("cuda", 2)


def test_class_array():
    arr, cl = A.class_array((3, np.int64(5), 19), 20, "no CAM")
    assert cl == [3, 5, 19] and list(arr) == cl and arr._type_.__name__ == "c_int"
    with pytest.raises(ValueError, match="no classes: an image without a positive class has no CAM"):
        A.class_array([], 20, "no CAM")
    for bad, word in (([3, 20], "outside 0..19"), ([-1, 3], "outside 0..19"), ([5, 3], "ascending"), ([3, 3], "ascending")):
        with pytest.raises(ValueError, match=word):
            A.class_array(bad, 20, "no CAM")


def test_workspace_raises_the_library_s_refusal_before_it_allocates():
    for device in ("cuda", "cpu"):
        with pytest.raises(L.AcrHipError) as e:
            L.workspace("acr_featdis_ws_bytes", 0, 21, 8, 4, 4, device=device)
        assert "acr_featdis_ws_bytes" in str(e.value) and "B=0" in str(e.value)
    lib = L.load()
    for dtype, size in ((torch.uint8, 1), (torch.float32, 4), (torch.float64, 8)):       # a good query: the size asked for, in elements
        ws, nbytes = L.workspace("acr_featdis_ws_bytes", 2, 21, 8, 4, 4, device="cpu", dtype=dtype)
        assert nbytes == lib.acr_featdis_ws_bytes(2, 21, 8, 4, 4) > 0 and nbytes % 8 == 0
        assert ws.dtype == dtype and ws.numel() * size == nbytes
