"""CPU: the scene-level FeatureNet cache (damvs_feature_gather, scene.SceneFeatures, CascadeMVSNet.forward(features=),
reconstruct_scene(features="scene")) without a GPU.

  * the C entry point's validation: every DAMVS_E_ARG / DAMVS_E_SHAPE case comes back before any device work, with a
    message that names the argument;
  * the binding, the header's constants and the package's exports;
  * the ValueErrors of the Python layer that need no device.
"""
import ctypes
import os

import pytest
import torch

E_ARG, E_SHAPE = -1, -2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from damvsnet_amd import _capi, build
    build.build()
    return _capi.load_library()


def ptrs(*v):
    return (ctypes.c_void_p * len(v))(*v)


def sizes(*v):
    return (ctypes.c_ulonglong * len(v))(*v)


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_feature_gather_validates_before_device_work(lib):
    P = 256  # never dereferenced: every call below fails validation

    def call(n=3, K=2, V=6, stores=(P, P + 16), vb=(16, 4096), slots=(5, 0, 5), outs=(P + 32, P + 48)):
        return lib.damvs_feature_gather(None, n, K, V, stores if stores is None else ptrs(*stores),
                                        vb if vb is None else sizes(*vb), slots if slots is None else ints(*slots),
                                        outs if outs is None else ptrs(*outs))

    err = lambda: lib.damvs_last_error_string()
    # null pointers and alignment: DAMVS_E_ARG
    assert call(stores=None) == E_ARG and b"null stores" in err()
    assert call(vb=None) == E_ARG and b"null view_bytes" in err()
    assert call(slots=None) == E_ARG and b"null slots" in err()
    assert call(outs=None) == E_ARG and b"null outs" in err()
    assert call(stores=(P, None)) == E_ARG and b"null stores[1]" in err()
    assert call(outs=(None, P)) == E_ARG and b"null outs[0]" in err()
    for off in (1, 4, 8):
        assert call(stores=(P, P + off)) == E_ARG and b"stores[1]" in err() and b"16-byte aligned" in err()
        assert call(outs=(P + off, P)) == E_ARG and b"outs[0]" in err() and b"16-byte aligned" in err()
    # counts: DAMVS_E_SHAPE
    for n in (0, -1, 129):
        assert call(n=n, slots=[0] * 129) == E_SHAPE and b"n_pairs %d" % n in err() and b"128" in err()
    for K in (0, -2, 5):
        assert call(K=K, stores=[P] * 5, vb=[16] * 5, outs=[P] * 5) == E_SHAPE and b"K %d" % K in err()
    for V in (0, -3):
        assert call(V=V) == E_SHAPE and b"V %d" % V in err()
    # slots
    assert call(slots=(5, 6, 2)) == E_SHAPE and b"slot 6 of pair 1" in err()
    assert call(slots=(-1, 0, 2)) == E_SHAPE and b"slot -1 of pair 0" in err()
    assert call(V=5) == E_SHAPE and b"slot 5 of pair 0" in err() and b"[0, 5)" in err()
    # view_bytes
    assert call(vb=(16, 0)) == E_SHAPE and b"view_bytes[1] is 0" in err()
    for bad in (8, 24, 4097):
        assert call(vb=(bad, 16)) == E_SHAPE and b"view_bytes[0] %d" % bad in err() and b"multiple of 16" in err()
    assert call(vb=(16, 2 ** 31)) == E_SHAPE and b"view_bytes[1] 2147483648" in err() and b"2^31" in err()
    assert call(vb=(2 ** 40, 16)) == E_SHAPE and b"2^31" in err()
    # the first fault found is the one reported, tensor by tensor: tensor 0's size before tensor 1's pointer
    assert call(vb=(24, 16), stores=(P, None)) == E_SHAPE and b"view_bytes[0] 24" in err()


def test_binding_and_exports():
    import damvsnet_amd
    from damvsnet_amd import _capi, scene
    assert damvsnet_amd.SceneFeatures is scene.SceneFeatures and "SceneFeatures" in damvsnet_amd.__all__
    assert "damvs_feature_gather" in [s[0] for s in _capi.SIGNATURES]
    assert _capi.FEATURES_MAX_PAIRS == 128 and _capi.FEATURES_MAX_TENSORS == 4
    header = open(os.path.join(REPO, "include", "damvs.h")).read()
    assert "#define DAMVS_FEATURES_MAX_PAIRS 128" in header and "#define DAMVS_FEATURES_MAX_TENSORS 4" in header


def test_reconstruct_scene_refuses_an_unknown_features_mode_before_touching_the_model(tmp_path):
    from damvsnet_amd.scene import reconstruct_scene
    ply = str(tmp_path / "never.ply")
    for bad in ("x", "device", None, True):
        with pytest.raises(ValueError, match="features must be"):
            reconstruct_scene(None, str(tmp_path), "scan1", ply, features=bad)
        with pytest.raises(ValueError, match="features must be"):
            reconstruct_scene(None, str(tmp_path), "scan1", ply, inputs="device", features=bad)
    assert not os.path.exists(ply)


def test_scene_features_refuses_the_torch_front_end_and_bad_arguments():
    from damvsnet_amd.cascade import CascadeMVSNet
    from damvsnet_amd.scene import SceneFeatures
    net = CascadeMVSNet(ndepths=[8, 8, 8], frontend_impl="torch")
    with pytest.raises(ValueError, match="frontend_impl"):
        SceneFeatures(net, [0, 1], 64, 96, "cpu")
    hip = CascadeMVSNet(ndepths=[8, 8, 8])
    with pytest.raises(ValueError, match="distinct"):
        SceneFeatures(hip, [0, 1, 0], 64, 96, "cpu")
    with pytest.raises(ValueError, match="distinct"):
        SceneFeatures(hip, [], 64, 96, "cpu")
    for H, W in ((0, 96), (64, 98), (62, 96)):
        with pytest.raises(ValueError, match="multiples of 4"):
            SceneFeatures(hip, [0, 1], H, W, "cpu")


def test_forward_refuses_features_with_the_torch_front_end():
    from damvsnet_amd.cascade import CascadeMVSNet
    net = CascadeMVSNet(ndepths=[8, 8, 8], frontend_impl="torch").eval()
    with pytest.raises(ValueError, match="frontend_impl"):
        net(torch.zeros(1, 1, 3, 64, 64), {}, torch.zeros(1, 8), features=[{}])
