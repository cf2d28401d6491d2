"""lvk::draw_points / draw_rect / draw_text and StabilizationFilter::draw_hud of the C++ facade (include/lvk/Drawing.hpp, driven by
tests/cpp/drawing_facade.cpp): each function with its default arguments against tests/np_draw.py, and draw_hud on a frame the stabilizer
emitted against the composition of the specification's calls.  CPU: it compiles and refuses bad arguments; GPU: it draws."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import np_draw as nd
from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "drawing_facade.cpp")
COLOUR = (7, 200, 99)
# Drawing.hpp:23-71, indexed by VideoFrame::Format
GREEN = {0: (0, 255, 0), 4: (149, 43, 21)}
RED = {0: (0, 0, 255), 4: (76, 84, 255)}
MAGENTA = {0: (255, 0, 255), 4: (105, 212, 234)}


def test_facade_drawing_compiles(tmp_path):
    build_facade(tmp_path, SRC)


def test_facade_refuses_bad_arguments(tmp_path):
    exe = build_facade(tmp_path, SRC)
    r = subprocess.run([exe, "refuse"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "refuse ok: 5 refused" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(135, 240), (1080, 1920)])
def test_facade_defaults(tmp_path, rows, cols):
    exe = build_facade(tmp_path, SRC)
    img = np.random.default_rng(rows).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    img.tofile(tmp_path / "frame.bin")
    r = subprocess.run([exe, "defaults", str(rows), str(cols), str(tmp_path / "frame.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "defaults ok: 4 frames" in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(4, rows, cols, 3)
    # the reference's defaults: point_size = 10, thickness = 2, font_scale = 1.5 (-> blocks of 3), font_thickness = 2
    pts = [(10.5, 20.25), (0, 0), (cols, rows), (100.5, 50.5), (-30, 7)]
    assert np.array_equal(got[0], nd.points(img, pts, COLOUR, 10))
    assert np.array_equal(got[1], nd.rect(img, (30, 20, 100, 60), COLOUR, 2))
    assert np.array_equal(got[2], nd.text(img, "LVK 0.12ms {~}", (12, 60), COLOUR, nd.font_scale_to_scale(1.5), 2))
    want = nd.text(nd.rect(img, (30, 22, 100, 60), COLOUR, 2), "Rect2f", (41, 70), COLOUR, 3, 2)
    assert np.array_equal(got[3], want)
    for g in got:
        assert not np.array_equal(g, img)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,frame_time_ms,deviation_ms", [(4, 4.25, 0.5), (0, 7.5, 12.345)])
def test_facade_draw_hud_on_a_stabilized_frame(tmp_path, fmt, frame_time_ms, deviation_ms):
    from tests import synth
    exe = build_facade(tmp_path, SRC)
    rows, cols, n = 270, 480, 6
    clip, _ = synth.make_clip(rows, cols, n, seed=23)
    with open(tmp_path / "clip.bin", "wb") as f:
        for fr in clip:
            f.write(np.ascontiguousarray(fr).tobytes())
    r = subprocess.run([exe, "hud", str(fmt), str(rows), str(cols), str(n), repr(frame_time_ms), repr(deviation_ms), str(tmp_path / "clip.bin"),
                        str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    m = re.search(r"hud ok: region (-?\d+) (-?\d+) (-?\d+) (-?\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout, r.stderr)
    x, y, w, h = (int(v) for v in m.groups())
    assert 0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= cols and y + h <= rows
    before, after = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(2, rows, cols, 3)
    # VSFilter::draw_debug_hud (VSFilter.cpp:368-383): the text first, then the rectangle, both with the reference's default arguments
    text = "%.2fms (%.2fms)" % (frame_time_ms, deviation_ms)
    colour = GREEN[fmt] if frame_time_ms < 6.0 else RED[fmt]
    want = nd.rect(nd.text(before, text, (x + 5, y + 40), colour, 3, 2), (x, y, w, h), MAGENTA[fmt], 2)
    assert np.array_equal(after, want)
    assert not np.array_equal(after, before)
