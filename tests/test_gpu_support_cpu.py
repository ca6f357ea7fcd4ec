"""tests/gpu_support.py, the GPU modules' shared scaffolding, without a GPU: the environment knobs come back, the samplings are
the two meanings the modules use, the comparisons name the element that differs, and the CLI preamble is the text the modules
used to spell out by hand."""
import os
import types

import numpy as np
import pytest

import gpu_support as gs
import segment_cases as sc


def test_env_sets_unsets_and_restores():
    os.environ["HMRM_T_KEEP"], os.environ["HMRM_T_DROP"] = "before", "there"
    os.environ.pop("HMRM_T_NEW", None)
    try:
        with gs.env(HMRM_T_KEEP=7, HMRM_T_DROP=None, HMRM_T_NEW="x"):
            assert os.environ["HMRM_T_KEEP"] == "7" and "HMRM_T_DROP" not in os.environ and os.environ["HMRM_T_NEW"] == "x"
            with gs.env(HMRM_T_NEW=None):  # (unsetting what is not set is no error either)
                assert "HMRM_T_NEW" not in os.environ
            assert os.environ["HMRM_T_NEW"] == "x"
        assert os.environ["HMRM_T_KEEP"] == "before" and os.environ["HMRM_T_DROP"] == "there" and "HMRM_T_NEW" not in os.environ
        with pytest.raises(KeyError):
            with gs.env(HMRM_T_KEEP="during", HMRM_T_DROP=None, HMRM_T_NEW=1):
                raise KeyError("the body raises")
        assert os.environ["HMRM_T_KEEP"] == "before" and os.environ["HMRM_T_DROP"] == "there" and "HMRM_T_NEW" not in os.environ
    finally:
        for k in ("HMRM_T_KEEP", "HMRM_T_DROP", "HMRM_T_NEW"):
            os.environ.pop(k, None)


def test_kernel_variant_none_is_the_scenes_own_choice():
    with gs.env(HMRM_KERNEL="group"):
        with gs.kernel_variant(None):
            assert "HMRM_KERNEL" not in os.environ
            with gs.kernel_variant("rec"):
                assert os.environ["HMRM_KERNEL"] == "rec"
        assert os.environ["HMRM_KERNEL"] == "group"


def test_samplings_of_both_meanings():
    assert gs.KERNEL_VARIANTS == ("leap", "group", "simple", "rec") and gs.SAMPLINGS == (0, 1, 2)
    assert [gs.samplings_of(v) for v in gs.KERNEL_VARIANTS] == [(0, 1, 2), (0, 1, 2), (0, 1, 2), (0,)]
    assert [gs.samplings_of(v, nearest_only=("rec", "simple")) for v in gs.KERNEL_VARIANTS] == [(0, 1, 2), (0, 1, 2), (0,), (0,)]
    assert gs.samplings_of(None) == (0, 1, 2)  # (the scene's own choice)


def test_same_frame_names_the_pixel():
    want = (np.arange(5 * 7 * 4) % 251).astype(np.uint8).reshape(5, 7, 4)
    gs.same_frame(want.copy(), want, "equal")
    gs.same_frame(want.copy(), want.reshape(35, 4), "equal, flat")
    got = want.copy()
    got[3, 2, 1] ^= 1
    got[4, 6, 0] ^= 1
    with pytest.raises(AssertionError, match=r"planted: 2 of 35 pixels differ; first \(2, 3\): got ") as e:
        gs.same_frame(got, want.reshape(35, 4), "planted")
    assert str(e.value).endswith(f"got {got[3, 2]}, want {want[3, 2]}")


def test_same_records_names_the_field_and_the_ray():
    dt = np.dtype([("point", np.float64, 3), ("steps", np.uint32), ("status", np.uint8)], align=True)
    want = np.zeros(9, dtype=dt)
    want["point"] = np.arange(27).reshape(9, 3)
    want["steps"] = np.arange(9)

    def twin():  # (ndarray.copy() copies field by field and leaves the padding to chance)
        return np.frombuffer(bytearray(want.tobytes()), dtype=dt)

    gs.same_records(twin(), want, "equal")
    got = twin()
    got["steps"][[4, 6]] += 1
    with pytest.raises(AssertionError, match=r"planted: field 'steps' differs for 2 of 9 rays; first 4: got ") as e:
        gs.same_records(got, want, "planted")
    assert str(e.value).endswith(f"got {got[4]}, want {want[4]}")
    got = twin()
    got["point"][7, 2] = -0.0 if want["point"][7, 2] == 0.0 else -want["point"][7, 2]
    with pytest.raises(AssertionError, match=r"field 'point' differs for 1 of 9 rays; first 7"):
        gs.same_records(got, want, "planted")
    got = twin()
    got.view(np.uint8).reshape(9, dt.itemsize)[2, dt.fields["status"][1] + 1] = 1  # (a byte no field owns)
    with pytest.raises(AssertionError, match="records differ in padding"):
        gs.same_records(got, want, "planted")


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_same_cells_names_the_cell(dtype):
    want = (np.arange(6 * 11) % 200).reshape(6, 11)  # (the replay's sums come in a wider type)
    gs.same_cells(want.astype(dtype), want, "equal", dtype)
    gs.same_cells(want.astype(dtype), want.astype(dtype), "equal, same type", dtype)
    got = want.astype(dtype)
    got[2, 9] += 1
    with pytest.raises(AssertionError, match=r"planted: 1 of 66 cells differ; first \(9, 2\): got " + f"{got[2, 9]}, want {want[2, 9]}"):
        gs.same_cells(got, want, "planted", dtype)
    other = np.uint16 if dtype == np.uint8 else np.uint8
    with pytest.raises(AssertionError):
        gs.same_cells(want.astype(other), want, "another type", dtype)
    with pytest.raises(AssertionError):
        gs.same_cells(want.astype(dtype)[:, :10], want, "another shape", dtype)


@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
def test_cli_config_is_the_old_literal(hmrm, tmp_path, inside):
    gw = 0.5
    rgb, cmap = sc.maps()
    world = types.SimpleNamespace(rgb=rgb, cmap=cmap)
    cfgp, text, outp = gs.cli_config(hmrm, world, tmp_path, gw, inside=inside, extra="interior on\n")
    hp, cp = str(tmp_path / "h.ppm"), str(tmp_path / "c.png")
    assert outp == str(tmp_path / "frame.png") and cfgp == tmp_path / "c.txt"
    # the text the GPU modules carried, pasted: test_lit_gpu.py's (outside) and test_geometry_gpu.py's (inside) position
    if inside:
        pos = (20.0 * gw, -20.0 * gw, 7.5 * gw)
        old = (f"resolution 40 30\nhfov 80\nhang -50\nvang 112\npos {pos[0]:.17g} {pos[1]:.17g} {pos[2]:.17g}\n"
               f"min_height 0.0\nmax_height {8.0 * gw:.17g}\ngrid_width {gw:.17g}\nstep_dist {0.2 * gw:.17g}\nbg_color 12 34 56\ncycle 1\n"
               f"projection perspective\nheightmap {hp}\ncolormap {cp}\noutput {outp}\n")
    else:
        old = (f"resolution 40 30\nhfov 80\nhang -50\nvang 112\npos {-6.0 * gw:.17g} {8.0 * gw:.17g} {14.0 * gw:.17g}\n"
               f"min_height 0.0\nmax_height {8.0 * gw:.17g}\ngrid_width {gw:.17g}\nstep_dist {0.2 * gw:.17g}\nbg_color 12 34 56\ncycle 1\n"
               f"projection perspective\nheightmap {hp}\ncolormap {cp}\noutput {outp}\n")
    assert text == old
    assert text.startswith("resolution 40 30\nhfov 80\nhang -50\nvang 112\npos " + ("10 -10 3.75\n" if inside else "-3 4 7\n"))
    assert cfgp.read_text() == old + "interior on\n"
    assert hmrm.image_load(hp, 3)[0].tobytes() == rgb.tobytes() and hmrm.image_load(cp, 4)[0].tobytes() == cmap.tobytes()
    # the variants three modules need: no output line, another frame size, the spherical inside camera of test_segments_gpu.py
    _, bare, _ = gs.cli_config(hmrm, world, tmp_path, gw, inside=inside, output=False, width=20, height=15)
    assert bare == old.replace("resolution 40 30\n", "resolution 20 15\n").replace(f"output {outp}\n", "")
    _, sph, _ = gs.cli_config(hmrm, world, tmp_path, gw, inside=inside, proj=2)
    assert sph == old.replace("hfov 80\n", "hfov 150\n").replace("projection perspective\n", "projection spherical\n")
    # ... and the numbers are the camera's own: all but the orthographic width, which the preamble never named
    cam, cfg = sc.camera(hmrm, gw, 2, inside), hmrm.Config().consume_string(sph)
    try:
        cam.ortho_width = cfg.camera().ortho_width
        assert bytes(cfg.camera()) == bytes(cam)
        assert bytes(cfg.scene_params()) == bytes(sc.scene_params(hmrm, gw))
    finally:
        cfg.close()
