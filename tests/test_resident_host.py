"""DeviceMatrix and the device-resident form of an InfercnvObject (DESIGN K32) without a GPU: the class accepts CPU tensors,
so its shape, layout, counters and refusals are checked here; what runs on the device is in tests/test_gpu_resident.py."""
import inspect
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import infercnv_amd                                                     # noqa: E402
from infercnv_amd import DeviceMatrix, GeneOrder, InfercnvObject        # noqa: E402


def _obj(G=7, C=5, hspike=True):
    rng = np.random.default_rng(3)
    x = np.asfortranarray(rng.standard_normal((G, C)))
    x[0, 0], x[1, 2] = -0.0, 5e-324
    o = InfercnvObject(x, GeneOrder(np.array(["chr1"] * 4 + ["chr2"] * (G - 4)), np.arange(G), np.arange(G) + 1),
                       reference_grouped_cell_indices={"n": np.array([0, 1], dtype=np.int32)},
                       observation_grouped_cell_indices={"t": np.arange(2, C, dtype=np.int32)},
                       count_data=np.arange(G * C).reshape(G, C), options={"a": 1})
    if hspike:
        o.hspike = _obj(4, 3, hspike=False)
    return o


def test_shape_tensor_and_host_layout():
    x = np.asfortranarray(np.arange(12, dtype=np.float64).reshape(3, 4))      # G = 3 genes, C = 4 cells
    dm = DeviceMatrix(torch.from_numpy(np.ascontiguousarray(x.T)), "expr")
    assert dm.shape == (3, 4) and dm.ndim == 2 and dm.size == 12 and dm.nbytes == 96 and dm.kind == "expr"
    assert tuple(dm.tensor.shape) == (4, 3) and dm.tensor.dtype == torch.float64
    assert dm.float_tensor() is dm.tensor
    h = dm.to_host()
    assert h.shape == (3, 4) and h.dtype == np.float64 and h.flags.f_contiguous
    assert np.array_equal(h.view(np.uint64), x.view(np.uint64))
    h[0, 0] = 99.0                                                            # a copy: the matrix is left alone
    assert float(dm.tensor[0, 0]) == 0.0


def test_states_255_becomes_minus_one():
    st = np.array([[1, 255, 3], [6, 2, 255]], dtype=np.uint8)                 # (C = 2, G = 3)
    dm = DeviceMatrix(torch.from_numpy(st), "states")
    assert dm.shape == (3, 2)
    h = dm.to_host()
    assert h.dtype == np.float64 and h.flags.f_contiguous
    assert np.array_equal(h, np.array([[1, 6], [-1, 2], [3, -1]], dtype=np.float64))
    assert np.array_equal(dm.float_tensor().numpy(), h.T)
    back = DeviceMatrix.from_host(h, "states", device="cpu")                  # -1 -> 255 on the way in
    assert torch.equal(back.tensor, dm.tensor)


def test_constructor_refusals():
    t = torch.zeros((2, 3), dtype=torch.float64)
    with pytest.raises(ValueError):
        DeviceMatrix(t, "counts")
    with pytest.raises(TypeError):
        DeviceMatrix(t, "states")                                             # states are uint8
    with pytest.raises(TypeError):
        DeviceMatrix(t.to(torch.float32))
    with pytest.raises(TypeError):
        DeviceMatrix(t.T)                                                     # not contiguous
    with pytest.raises(TypeError):
        DeviceMatrix(np.zeros((2, 3)))
    with pytest.raises(TypeError):
        DeviceMatrix(torch.zeros(6, dtype=torch.float64))


def test_array_conversion_raises_and_names_to_host():
    dm = DeviceMatrix(torch.zeros((2, 3), dtype=torch.float64))
    for convert in (np.asarray, np.array, lambda m: np.asfortranarray(m, dtype=np.float64), lambda m: np.isnan(m)):
        with pytest.raises(TypeError, match=r"to_host\(\)"):
            convert(dm)


def test_counters_count_both_ways():
    DeviceMatrix.stats(reset=True)
    assert DeviceMatrix.stats() == {"uploads": 0, "fetches": 0, "bytes_up": 0, "bytes_down": 0}
    dm = DeviceMatrix.from_host(np.zeros((3, 4)), device="cpu")
    DeviceMatrix(torch.zeros((2, 2), dtype=torch.float64))                    # wrapping a tensor is no crossing
    assert DeviceMatrix.stats() == {"uploads": 1, "fetches": 0, "bytes_up": 96, "bytes_down": 0}
    dm.to_host()
    DeviceMatrix(torch.zeros((5, 2), dtype=torch.uint8), "states").to_host()
    assert DeviceMatrix.stats(reset=True) == {"uploads": 1, "fetches": 2, "bytes_up": 96, "bytes_down": 96 + 10}
    assert DeviceMatrix.stats()["fetches"] == 0


def test_object_round_trip_is_bit_equal_hspike_included():
    o = _obj()
    DeviceMatrix.stats(reset=True)
    r = o.to_device("cpu")
    assert r.is_resident() and r.hspike.is_resident() and not o.is_resident()
    assert isinstance(r.expr_data, DeviceMatrix) and r.expr_data.shape == o.expr_data.shape
    assert r.count_data is o.count_data and r.hspike.count_data is o.hspike.count_data      # counts and metadata stay
    assert r.gene_order is o.gene_order and r.options is o.options
    assert r.validate() and r.copy().expr_data is r.expr_data
    assert list(r.genes()) == list(o.genes()) and list(r.cells()) == list(o.cells())
    assert r.to_device("cpu").expr_data is r.expr_data                                      # already resident: as it is
    h = r.to_host()
    for a, b in ((h.expr_data, o.expr_data), (h.hspike.expr_data, o.hspike.expr_data)):
        assert isinstance(a, np.ndarray) and a.flags.f_contiguous and a.dtype == np.float64
        assert np.array_equal(a.view(np.uint64), np.asarray(b).view(np.uint64))             # -0.0 and the subnormal included
    assert DeviceMatrix.stats() == {"uploads": 2, "fetches": 2, "bytes_up": 8 * (35 + 12), "bytes_down": 8 * (35 + 12)}
    assert o.to_host().expr_data is o.expr_data                                              # a host object: as it is


def test_validate_refuses_on_both_forms():
    o = _obj(hspike=False)
    o.reference_grouped_cell_indices = {"n": np.array([0, 9])}
    for form in (o, o.to_device("cpu")):
        with pytest.raises(ValueError):
            form.validate()


def test_unwired_entries_fail_loudly():
    """sample_object is out of scope for resident objects: it must stop at __array__, not fetch."""
    from infercnv_amd import sampling
    r = _obj(hspike=False).to_device("cpu")
    DeviceMatrix.stats(reset=True)
    with pytest.raises(TypeError, match=r"to_host\(\)"):
        sampling.sample_object(r, n_cells=2)
    assert DeviceMatrix.stats()["fetches"] == 0


def test_gates_take_a_states_matrix():
    from infercnv_amd.pipeline import states_not_constant
    const = DeviceMatrix(torch.full((4, 3), 3, dtype=torch.uint8), "states")
    assert states_not_constant(const) is False and states_not_constant(const.to_host()) is False
    t = const.tensor.clone()
    t[2, 1] = 255
    varied = DeviceMatrix(t, "states")
    assert states_not_constant(varied) is True and states_not_constant(varied.to_host()) is True
    assert states_not_constant(DeviceMatrix(torch.zeros((0, 3), dtype=torch.uint8), "states")) is True


def test_run_signature_is_untouched(golden_dir):
    assert "DeviceMatrix" in infercnv_amd.__all__
    want = json.load(open(os.path.join(golden_dir, "run_formals.json")))["run"]
    params = inspect.signature(infercnv_amd.run).parameters
    positional = [n for n, p in params.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == [n.replace(".", "_") for n in want["formals"]]         # residency comes from the object's type:
    assert [n for n in params if n not in positional] == ["seed", "on_step"]    # no argument was added for it
