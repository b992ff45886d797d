"""The size queries of the suppression family are host arithmetic over one layout statement each (cvx_carver, csrc/cvx_common.h): on a
small grid they return no more than the parent commit did (tests/golden/workspace_bytes_parent.json, recorded from its library), 0
exactly where it returned 0, and no less than the arrays' plain sizes as the sources document them.  No GPU is needed."""
import ctypes
import json
import os

import pytest

from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_bytes_parent.json")))
NMS_CAP, MERGE_CAP, CN_CAND_CAP, REGION_HEAD = 16384, 8192, 2048, 64


def nms_cap(a):
    c = 64
    while c < a and c < NMS_CAP:
        c <<= 1
    return c


# the arrays' plain sizes in bytes, without alignment or slack
PLAIN = {
    # per candidate two boxes, score, class, anchor index = 44 bytes, and a row of the suppression matrix, cap / 64 words
    "cvx_nms_workspace_bytes": lambda b, a: b * nms_cap(a) * (44 + nms_cap(a) // 8),
    "cvx_soft_nms_workspace_bytes": lambda b, a: b * nms_cap(a) * 44,
    "cvx_det_merge_workspace_bytes": lambda f: f * MERGE_CAP * (28 + MERGE_CAP // 8),                  # 28 per slot plus the matrix
    "cvx_det_wbf_workspace_bytes": lambda f: f * MERGE_CAP * (2 * 28 + 56),                            # two candidate tables, the cluster slots
    "cvx_seg_regions_workspace_bytes": lambda f, h, w: f * (28 * h * w + 4 * (REGION_HEAD + MERGE_CAP)),   # 28 per pixel, the candidates
    "cvx_centernet_decode_workspace_bytes": lambda b, h, w, c: b * (4 * h * w * c + 8 * CN_CAND_CAP),  # the peak scores, the slices' lists
    "cvx_loss_v8_workspace_bytes": lambda b, a, nc, n: 0,                                              # its own layout; the parent bounds it
}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(L.LIB_PATH), "build() leaves the cross-compiled library in the tree"
    return ctypes.CDLL(L.LIB_PATH)


def test_the_grid_is_the_one_the_parent_was_recorded_on():
    ns, anchors = [0, 1, 2, 32], [1, 63, 64, 65, 129, 8400, 16384, 20000]
    assert set(PARENT) == set(PLAIN)
    for name in ("cvx_nms_workspace_bytes", "cvx_soft_nms_workspace_bytes"):
        assert [p[:-1] for p in PARENT[name]] == [[b, a] for b in ns for a in anchors]
    for name in ("cvx_det_merge_workspace_bytes", "cvx_det_wbf_workspace_bytes"):
        assert [p[:-1] for p in PARENT[name]] == [[f] for f in ns]
    assert [p[:-1] for p in PARENT["cvx_seg_regions_workspace_bytes"]] == [[f, h, w] for f in ns for h, w in ((1, 1), (33, 65), (1024, 2048))]
    assert [p[:-1] for p in PARENT["cvx_centernet_decode_workspace_bytes"]] == [[b, h, w, c] for b in ns for h, w, c in ((8, 8, 3), (128, 128, 20))]


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_sizes_against_the_parent_and_the_plain_sum(lib, name):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int32] * (len(PARENT[name][0]) - 1)
    assert fn.argtypes == L.PROTOTYPES[name][1]
    for *args, parent in PARENT[name]:
        new = fn(*args)
        print(f"{name}{tuple(args)}: parent {parent}, new {new}, plain {PLAIN[name](*args)}")
        assert new <= parent, (name, args, new, parent)
        assert (new == 0) == (parent == 0), (name, args, new, parent)
        if new:
            assert new >= PLAIN[name](*args), (name, args, new)


def test_what_the_entries_refuse_stays_zero(lib):
    for name, refused in (("cvx_soft_nms_workspace_bytes", [(0, 5), (5, 0), (-1, 5)]), ("cvx_det_wbf_workspace_bytes", [(0,), (-3,)]),
                          ("cvx_seg_regions_workspace_bytes", [(0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 65536, 32768)])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int32] * len(refused[0])
        assert [fn(*a) for a in refused] == [0] * len(refused), name
