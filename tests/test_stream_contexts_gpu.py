"""Launch state per stream (csrc/api_internal.hpp StreamCtx) now that nothing is recorded behind a frame on a caller's stream: the
same pixels whichever stream a frame is launched on, the launch-order calibration of a caller's stream while the scene's
ticket lanes are busy (others_idle asks those streams directly), and the recycling of a stream's state -- behind a device
synchronisation -- when a scene is driven from more streams than it keeps state for, with work in flight on a stream whose
handle the caller has dropped.  Every frame is compared byte for byte with hmrm_render_stats' frame of the same camera."""
from importlib import import_module

import numpy as np
import pytest

import scenes
from gpu_support import gpu

pytestmark = pytest.mark.gpu

MAP = 64
MAX_STREAM_CTX = 32  # api_internal.hpp kMaxStreamCtx


@pytest.fixture()
def scene(gpu):
    rgb, cmap = scenes.small_maps(MAP, MAP, 811)
    s = gpu.Scene(rgb, cmap, gpu.SceneParams.make(0.0, 12.0, grid_width=1.0))
    yield s
    s.close()


def spherical(gpu, width=64, height=192):
    """12 tile rows of 16 pixels: the smallest frame whose launch order is calibrated (api_launch.cpp launch_frame)."""
    return gpu.Camera.make(width=width, height=height, projection=gpu.SPHERICAL, hfov=gpu.degrees_to_rads(160), hang=0.0,
                           vang=gpu.degrees_to_rads(110), pos=(-20.0, 20.0, 30.0), step_dist=0.25, bg=(1, 2, 3))


def perspective(gpu, width=48, height=32, k=0, n=1):
    base = gpu.Camera.make(width=width, height=height, projection=gpu.PERSPECTIVE, hfov=gpu.degrees_to_rads(80), hang=0.0,
                           vang=gpu.degrees_to_rads(115), pos=(-20.0, 20.0, 30.0), step_dist=0.25, bg=(4, 5, 6))
    return gpu.orbit_camera(base, MAP / 2.0, -MAP / 2.0, 70.0, gpu.degrees_to_rads(-45.0), k, n) if n > 1 else base


def device_frame(torch, cam):
    return torch.zeros((cam.height, cam.width, 4), dtype=torch.uint8, device="cuda")


def test_same_pixels_on_every_stream(gpu, scene):
    import torch
    for cam in (spherical(gpu), perspective(gpu)):
        want = scene.render_stats(cam)[0]
        assert np.array_equal(scene.render(cam), want)  # (the scene's own stream)
        own = torch.cuda.Stream()
        for handle in (own.cuda_stream, 0):  # a caller's stream, the null stream
            buf = device_frame(torch, cam)
            torch.cuda.synchronize()  # (the fill ran on torch's current stream)
            for _ in range(3):  # (again: from the cached record)
                scene.render_rows_device(cam, buf.data_ptr(), cam.width * 4, 0, cam.height, stream=handle)
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy(), want), (cam.projection, handle)
            assert scene.take_capped(handle) == 0


def test_calibration_with_ticket_lanes_busy(gpu, scene):
    """24 frames of one calibrated camera on a caller's stream -- more than its calibration measures -- while device tickets
    stay in flight on the scene's lanes: whether a launch may be measured is asked of those lanes' streams."""
    import torch
    lib = import_module("heightmap-ray-marcher_amd.lib").lib
    cam, tcam = spherical(gpu), perspective(gpu, 512, 512)
    want, twant = scene.render_stats(cam)[0], scene.render_stats(tcam)[0]
    caller = torch.cuda.Stream()
    frames = [device_frame(torch, cam) for _ in range(24)]
    tbufs = [device_frame(torch, tcam) for _ in range(6)]
    torch.cuda.synchronize()

    def one_pass():
        in_flight, seen = [], 0  # (ticket, buffer index)
        for k, buf in enumerate(frames):
            while len(in_flight) >= len(tbufs) - 1:
                t, b = in_flight.pop(0)
                scene.render_device_wait(t)
                assert np.array_equal(tbufs[b].cpu().numpy(), twant), ("ticket", seen)
                seen += 1
            for j in (2 * k, 2 * k + 1):
                in_flight.append((scene.render_device_begin(tcam, tbufs[j % len(tbufs)].data_ptr(), tcam.width * 4), j % len(tbufs)))
            scene.render_rows_device(cam, buf.data_ptr(), cam.width * 4, 0, cam.height, stream=caller.cuda_stream)
            if k % 2:  # (a measured launch is folded in once it has finished: let some finish)
                caller.synchronize()
        for t, b in in_flight:
            scene.render_device_wait(t)
            assert np.array_equal(tbufs[b].cpu().numpy(), twant), ("ticket", seen)
            seen += 1
        caller.synchronize()
        for k, buf in enumerate(frames):
            assert np.array_equal(buf.cpu().numpy(), want), ("frame", k)
            buf.zero_()
        torch.cuda.synchronize()
        assert seen == 2 * len(frames)
        assert scene.take_capped(caller.cuda_stream) == 0

    one_pass()
    assert lib.hmrm_debug_reload_env(scene._h) == gpu.HMRM_OK  # (forgets the calibration: the second pass measures again)
    one_pass()


def test_recycled_stream_state_with_work_in_flight(gpu, scene):
    """A frame in flight on a stream whose Python object is gone, then more streams than the scene keeps state for: the state
    of the least recently used stream is recycled behind a device synchronisation, and every frame still arrives."""
    import torch
    big = perspective(gpu, 512, 512)
    cams = [perspective(gpu, 64, 48, k, 64) for k in range(1, 42)]
    big_want = scene.render_stats(big)[0]
    want = [scene.render_stats(c)[0] for c in cams]
    big_buf = device_frame(torch, big)
    bufs = [device_frame(torch, c) for c in cams]
    torch.cuda.synchronize()
    first = torch.cuda.Stream()
    handles = {first.cuda_stream}
    scene.render_rows_device(big, big_buf.data_ptr(), big.width * 4, 0, big.height, stream=first.cuda_stream)
    del first
    # (torch hands out streams from one pool of 32 per priority: both priorities, so that the handles are distinct)
    streams = [torch.cuda.Stream(priority=-(k % 2)) for k in range(41)]
    for st, c, buf in zip(streams[:40], cams, bufs):
        handles.add(st.cuda_stream)
        scene.render_rows_device(c, buf.data_ptr(), c.width * 4, 0, c.height, stream=st.cuda_stream)
    assert len(handles) > MAX_STREAM_CTX, "the test needs more distinct streams than the scene keeps state for"
    torch.cuda.synchronize()
    assert np.array_equal(big_buf.cpu().numpy(), big_want)
    for k in range(40):
        assert np.array_equal(bufs[k].cpu().numpy(), want[k]), k
    last = streams[40]
    scene.render_rows_device(cams[40], bufs[40].data_ptr(), cams[40].width * 4, 0, cams[40].height, stream=last.cuda_stream)
    last.synchronize()
    assert np.array_equal(bufs[40].cpu().numpy(), want[40])
    assert scene.take_capped(last.cuda_stream) == 0
