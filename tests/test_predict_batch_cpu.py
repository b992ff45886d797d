"""CPU: the drawing rules of batched prediction -- the numpy restatement against answers worked out by hand, the label
text, the blend, the arg max -- and the plugin surface (``predict_batch`` / ``detect_frames`` on the five algorithm classes, no CPU path)."""
import numpy as np
import pytest
import torch

import builder
import check
from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import render as R
import render_restatement as RS


def art(text):
    return np.array([[c == "#" for c in line] for line in text.strip().split("\n")])


# box (3, 4) - (8, 9) on a 12 x 12 frame: every outline pixel, by hand, for thickness 1, 2, 3
OUTLINE = {
    1: """
............
............
............
............
...######...
...#....#...
...#....#...
...#....#...
...#....#...
...######...
............
............""",
    2: """
............
............
............
..########..
..########..
..##....##..
..##....##..
..##....##..
..##....##..
..########..
..########..
............""",
    3: """
............
............
............
..########..
..########..
..########..
..###..###..
..###..###..
..########..
..########..
..########..
............""",
}


@pytest.mark.parametrize("t", [1, 2, 3])
def test_outline_pixels_by_hand(t):
    row = [3.9, 4.2, 8.99, 9.5, 0.5, 0]                       # truncated towards zero: (3, 4) - (8, 9)
    outline, tag, text, cls = RS.box_layers(12, 12, row, thickness=t, font_scale=1)
    assert np.array_equal(outline, art(OUTLINE[t]))
    frame = np.full((12, 12, 3), 7, np.uint8)
    out, painted = RS.draw(frame, [row], 1, thickness=t, font_scale=1)
    only_outline = art(OUTLINE[t]) & ~tag
    assert (out[only_outline] == R.palette(2)[1]).all() and (out[~painted] == 7).all() and np.array_equal(painted, outline | tag)


def test_negative_coordinates_truncate_towards_zero():
    outline, _, _, _ = RS.box_layers(6, 6, [-0.9, -0.5, 2.7, 2.2, 0.5, 0], thickness=1, font_scale=1)     # (0, 0) - (2, 2), not (-1, -1)
    assert np.array_equal(outline[:4, :4], art("###.\n#.#.\n###.\n...."))


def test_later_box_wins_and_layer_order():
    frame = np.zeros((40, 60, 3), np.uint8)
    rows = [[5, 20, 30, 35, 0.9, 0], [20, 20, 50, 35, 0.8, 1]]
    out, _ = RS.draw(frame, rows, 2, thickness=1, font_scale=1)
    pal = R.palette(3)
    assert (out[35, 25] == pal[2]).all()                     # bottom edges overlap on x 20 .. 30: the later box's colour
    assert (out[35, 10] == pal[1]).all() and (out[35, 45] == pal[2]).all()
    # box 1's tag (rows 11 .. 19, from x 20) covers box 0's tag (from x 5) where they meet
    assert (out[11, 19] == pal[1].astype(int) * 7 // 10).all() and (out[11, 20] == pal[2].astype(int) * 7 // 10).all()
    first, _ = RS.draw(frame, rows, 1, thickness=1, font_scale=1)
    assert (first[35, 25] == pal[1]).all() and (first[25, 50] == 0).all()          # count = 1: the second row is not drawn
    # inside a box: text over tag over outline.  Box at the top edge: the tag starts at y0 and covers the outline's corner
    out, _ = RS.draw(frame, [[2, 3, 50, 30, 0.5, 0]], 1, thickness=1, font_scale=1)
    assert (out[3, 2] == pal[1].astype(int) * 7 // 10).all() and (out[3, 49] == pal[1]).all()


def test_tag_geometry_and_clipping_at_the_right_and_bottom_edges():
    # "1:50.0%" is 7 characters: the tag is (6 * 7 + 1) * fs wide and 9 * fs high
    _, tag, text, _ = RS.box_layers(40, 80, [10, 20, 30, 30, 0.5, 1], thickness=1, font_scale=1)
    want = np.zeros((40, 80), bool)
    want[11:20, 10:53] = True                                 # above the box: rows y0 - 9 .. y0 - 1
    assert np.array_equal(tag, want)
    glyph_1 = art(".....\n..#..\n.##..\n..#..\n..#..\n..#..\n..#..\n.###.\n.....")[1:8]       # the project's "1"
    assert np.array_equal(text[12:19, 11:16], glyph_1)
    colon = art(".....\n.##..\n.##..\n.....\n.##..\n.##..\n.....")
    assert np.array_equal(text[12:19, 17:22], colon) and not text[12:19, 16].any()           # one blank column between glyphs
    _, tag2, text2, _ = RS.box_layers(80, 160, [10, 20, 30, 30, 0.5, 1], thickness=1, font_scale=2)
    assert tag2.sum() == 86 * 18 and np.array_equal(text2[4:18:2, 12:22:2], glyph_1) and np.array_equal(text2[5:19:2, 13:23:2], glyph_1)
    # right edge: the tag starts at x0 = 70 of an 80 wide frame; bottom edge: y0 - 9 < 0 puts the tag inside the box, cut at row 11
    _, tag, _, _ = RS.box_layers(40, 80, [70, 20, 78, 30, 0.5, 1], thickness=1, font_scale=1)
    want = np.zeros((40, 80), bool)
    want[11:20, 70:80] = True
    assert np.array_equal(tag, want)
    _, tag, text, _ = RS.box_layers(12, 80, [4, 8, 30, 11, 0.5, 1], thickness=1, font_scale=1)
    want = np.zeros((12, 80), bool)
    want[8:12, 4:47] = True
    assert np.array_equal(tag, want) and np.array_equal(text[9:12, 5:10], glyph_1[:3])


def test_inverted_box_paints_nothing():
    frame = np.arange(20 * 20 * 3, dtype=np.uint8).reshape(20, 20, 3)
    for row in ([10, 5, 4, 15, 0.9, 1], [4, 15, 10, 5, 0.9, 1], [float("nan"), 1, 5, 5, 0.9, 1]):
        out, painted = RS.draw(frame, [row], 1)
        assert np.array_equal(out, frame) and not painted.any()
    out, painted = RS.draw(frame, [[5, 5, 5, 5, 0.9, 1]], 1, thickness=1, font_scale=1)        # x0 == x1: a one-pixel box still paints
    assert painted[5, 5]


def test_label_strings():
    assert R.format_label(0, np.float32(0.99949997)) == "0:99.9%"
    assert R.format_label(3, 0.25) == "3:25.0%"
    assert R.format_label(19, 0.0625) == "19:6.2%"            # 6.25 is exact: a tie, to even
    assert R.format_label(79, 1.0) == "79:100.0%"
    assert R.format_label(7, 0.001) == "7:0.1%"
    assert R.format_label(1, 0.1875) == "1:18.8%"             # 18.75: the other tie direction
    for s in (0.99949997, 0.25, 0.0625, 1.0, 0.001, 0.1875, 0.5555, 0.7):
        assert R.format_label(2, s) == "2:" + "{:.1f}".format(np.float32(s) * 100) + "%"
    assert R.format_label(-4, float("nan")) == "0:0.0%" and R.format_label(123456, 50.0) == "9999:999.9%"
    assert set(R.FONT) == set(R.GLYPHS) and all(len(g) == 7 and max(g) < 32 for g in R.FONT.values())


def test_palette_is_the_voc_colormap():
    from core.algorithms.segmentation_2d import voc_colormap
    p = R.palette(81)
    assert p.dtype == np.uint8 and p.shape == (81, 3) and [tuple(int(v) for v in c) for c in p[:21]] == voc_colormap()
    assert tuple(p[80]) == (32, 64, 0)                         # 80 = 0b1_010_000: round 1 gives G bit 6, round 2 gives R bit 5
    out, _ = RS.draw(np.zeros((40, 40, 3), np.uint8), [[5, 20, 30, 30, 0.5, 15]], 1, thickness=1, font_scale=1)
    assert (out[30, 20] == p[16]).all()                       # class c takes entry c + 1
    white = RS.draw(np.zeros((40, 80, 3), np.uint8), [[5, 20, 30, 30, 0.5, 0]], 1, thickness=1, font_scale=1)[0]
    assert (white[13, 6] == 255).all()                        # entry 1 = (128, 0, 0): sum 128 <= 382 -> white text (the "0"'s left stroke)
    black = RS.draw(np.zeros((40, 80, 3), np.uint8), [[5, 20, 30, 30, 0.5, 6]], 1, thickness=1, font_scale=1)[0]
    assert tuple(p[7]) == (128, 128, 128) and (black[11, 6] == 128 * 7 // 10).all() and (black[13, 7] == 0).all()    # sum 384 > 382 -> black


def test_blend_table_all_parities():
    # s = a + b: s % 4 == 0 -> s / 2; 1 -> down to the even half; 2 -> s / 2; 3 -> up to the even half
    assert RS.blend_half([4, 5, 6, 7, 0, 255, 255, 1], [0, 0, 0, 0, 0, 255, 254, 0]).tolist() == [2, 2, 3, 4, 0, 255, 254, 0]
    a, b = np.meshgrid(np.arange(256), np.arange(256))
    want = np.rint((a + b) / 2.0).astype(np.uint8)           # numpy's rint is round-half-even
    assert np.array_equal(RS.blend_half(a, b), want)


def test_argmax_ties_lowest_class():
    z = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 0.0, -2.0], [-3.0, -3.0, -4.0, -3.0]], np.float32).T
    assert RS.argmax_lowest(z, 0).tolist() == [1, 0, 0, 0]
    assert np.array_equal(RS.argmax_lowest(z, 0), torch.argmax(torch.from_numpy(z), 0).numpy())


def test_restated_resampling_matches_torch():
    """the restated taps against F.interpolate (bilinear, align_corners=False) on values where every step is exact, and the nearest rule"""
    z = np.arange(9 * 9 * 2, dtype=np.float32).reshape(81, 2) * 4
    got = RS.logits_at_network_size(z, 2, 9, 9, 36, 18)
    want = torch.nn.functional.interpolate(torch.from_numpy(z.reshape(9, 9, 2)).permute(2, 0, 1)[None], size=(36, 18), mode="bilinear")[0].numpy()
    assert np.allclose(got, want, rtol=1e-6, atol=1e-4)
    assert RS.nearest_index(4, 2).tolist() == [0, 0, 1, 1] and RS.nearest_index(3, 7).tolist() == [0, 2, 4] and RS.nearest_index(5, 5).tolist() == [0, 1, 2, 3, 4]
    a = np.float32([1.5, 3.0, 0.1]); b = np.float32([2.5, 1e-8, 0.3]); c = np.float32([0.25, 3.0, -0.03])
    assert RS._fma(a, b, c).tolist() == [4.0, float(np.float32(3.0 + 3e-8)), float(np.float32(np.float64(a[2]) * np.float64(b[2]) + np.float64(c[2])))]


# ---- plugin surface ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", check.MODELS)
def test_predict_batch_and_detect_frames_on_every_algorithm_class(name):
    from scripts import detect
    cfg, algo_cls, _ = builder.export_from_registry(name)
    assert callable(getattr(algo_cls, "predict_batch")) and callable(getattr(algo_cls, "detect_frames"))
    algo = algo_cls(cfg, torch.device("cpu"))
    frame = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(CvxError):
        algo.predict_batch(None, [frame])
    with pytest.raises(CvxError):
        algo.detect_frames(None, [frame], 1)
    with pytest.raises(CvxError):
        detect.detect_frames(algo, None, [frame], 1)
    assert callable(detect.detect_video)


def test_wrappers_refuse_host_tensors():
    frame = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(CvxError):
        R.FrameBatch([frame])
    with pytest.raises(CvxError):
        R.letterbox_batch([frame], (16, 16))
    with pytest.raises(CvxError):
        R.det_to_image(torch.zeros(1, 4, 6), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(CvxError):
        R.draw_detections([frame], torch.zeros(1, 4, 6), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(CvxError):
        R.seg_overlay([frame], torch.zeros(1, 4, 8), 3, (2, 2), (8, 8))
