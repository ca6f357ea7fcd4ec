"""What tests/test_geometry_cpu.py and tests/test_geometry_gpu.py share: a cache of replayed geometry planes
(tests/geometry_replay.py) on top of tests/lit_cases.py's primary records and camera rays -- the map, grid widths and cameras of
tests/segment_cases.py -- computed once per camera, read-only."""
import geometry_replay as gr
import lit_cases as lc
from lit_cases import BASE_CAP


class Replays(lc.Replays):
    def __init__(self, hmrm, oracle):
        super().__init__(hmrm, oracle)
        self._planes = {}

    def planes(self, gw, proj, sampling, inside=False, width=40, height=30, step_cap=BASE_CAP):
        """(planes, primary records) of segment_cases.camera(gw, proj, inside, sampling, width, height); inside: under the
        interior rule."""
        key = (gw, proj, sampling, inside, width, height, step_cap)
        if key not in self._planes:
            primary = self.primary(gw, proj, sampling, inside, width, height, step_cap)
            want = gr.planes(primary, self.rays(gw, proj, inside, width, height), self.heights[gw], self.params[gw], sampling)
            for v in want.values():
                v.setflags(write=False)
            self._planes[key] = (want, primary)
        return self._planes[key]
