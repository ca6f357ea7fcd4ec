"""What tests/test_lit_pipeline_cpu.py and tests/test_lit_pipeline_gpu.py share: the antialiased lit frame's definition
(include/hmrm.h hmrm_render_shaded_aa) from two things the CPU tests already pin to the oracle -- aa_box.box_filter of
shade_cases.Replays.shaded of the super frame -- the output shapes, and the content conditions of each: how many output pixels
have a block of samples that mixes hit with non-hit samples, and shadowed with unshadowed hit samples.  Those are the pixels
in which a kernel that filtered before shading, or shaded one sample per block, would differ."""

import lit_replay as lr
from aa_box import box_filter
from segment_cases import GRID_WIDTHS
from shade_cases import AMBIENT, SUNS  # noqa: F401

# (output width, output height, factor): the smallest at which this can go wrong
BASE = (20, 15, 2)  # super frame 40 x 30: the cached base replays; several workgroups, ragged tiles
OTHER_SHAPES = ((10, 8, 4),   # 40 x 32: ragged tiles
                (5, 4, 8),    # 40 x 32: one block per wave
                (52, 34, 2),  # 104 x 68: more than one workgroup each way, no multiple of the 8 x 16 tile
                (26, 17, 4))  # 104 x 68
# at least this many output pixels whose block mixes (hit and non-hit samples, shadowed and unshadowed hit samples)
MIN_MIXED = {BASE: (20, 10), (10, 8, 4): (8, 5), (5, 4, 8): (5, 4), (52, 34, 2): (40, 70), (26, 17, 4): (30, 45)}
# ... which the replay of bilinear sampling does not reach at 104 x 68 (its minima over every projection and sun are 50 and 34
# blocks mixing shadowed and unshadowed hits): what the replay alone gives.  Nearest and float thresholds: 78 and 50.
MIN_MIXED_BILINEAR = {(52, 34, 2): (40, 50), (26, 17, 4): (30, 34)}
MODES = ((True, True), (True, False), (False, True))  # (diffuse, shadows): shaded with shadows, shaded without, shadows only


def other_cases():
    """(shape, grid width, projection, sun) of the shapes beside the base one: grid width 0.5, 40 x 32 also at the other two;
    suns paired with projections."""
    for shape in OTHER_SHAPES:
        for gw in (GRID_WIDTHS if shape[0] * shape[2] == 40 else (0.5,)):
            for proj in (1, 2, 3):
                yield shape, gw, proj, SUNS[proj - 1]


def expected(replays, gw, proj, sampling, sun, diffuse, shadows, shape, **kw):
    """(the W x H antialiased lit frame, the replay of its super frame) of segment_cases.camera(gw, proj, ..., W, H)."""
    w, h, n = shape
    want = replays.shaded(gw, proj, sampling, sun, diffuse, shadows, width=n * w, height=n * h, **kw)
    return box_filter(want["rgba"].reshape(n * h, n * w, 4), n), want


def mixed_blocks(want, shape):
    """(output pixels whose n x n block holds hit and non-hit samples, ... shadowed and unshadowed hit samples)."""
    w, h, n = shape
    hit = (want["primary"]["status"] == lr.HIT).reshape(h, n, w, n)
    dark = hit & want["shadowed"].reshape(h, n, w, n)
    hits, darks = hit.sum(axis=(1, 3)), dark.sum(axis=(1, 3))
    return int(((hits > 0) & (hits < n * n)).sum()), int(((darks > 0) & (darks < hits)).sum())


def check_content(want, shape, sampling, shadows, what):
    mixed_hit, mixed_shadow = mixed_blocks(want, shape)
    need_hit, need_shadow = (MIN_MIXED_BILINEAR if sampling == 1 else MIN_MIXED).get(shape, MIN_MIXED[shape])
    assert mixed_hit >= need_hit, (what, shape, "blocks mixing hit and non-hit samples", mixed_hit)
    if shadows:
        assert mixed_shadow >= need_shadow, (what, shape, "blocks mixing shadowed and unshadowed hits", mixed_shadow)
    assert want["capped"] == 0, what
