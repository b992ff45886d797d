"""Host restatement (numpy) of what the input pipeline adds to ``csrc/augment.hip``: rendering without the colour transform
(``cvx_aug_images_plain``), the validation geometry, and the per-image regrouping of the box kernel's rows (``cvx_aug_boxes_padded``).  Built on
tests/aug_restatement.py; shared by tests/test_input_pipeline_cpu.py and tests/test_input_pipeline_gpu.py.
"""
import numpy as np

import aug_restatement as R

F = np.float32


def val_job(ih, iw, H, W):
    """get_random_data(random=False), detection_dataset.py:137-142, in Python floats like the reference"""
    scale = min(W / iw, H / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    return dict(ih=int(ih), iw=int(iw), nh=nh, nw=nw, dx=(W - nw) // 2, dy=(H - nh) // 2, flip=0, quad=-1, rect=(0, 0, W, H))


def render_plain(jobs, sources, H, W):
    """``R.render`` without its last step: paste + bicubic resize (+ the flips and the quadrant composition, which the kernel template shares
    with the colour path), bytes (H, W, 3)"""
    out = np.zeros((H, W, 3), np.uint8)
    for jb, src in zip(jobs, sources):
        assert src.shape[:2] == (jb["ih"], jb["iw"])
        mosaic = jb["quad"] >= 0
        pic = R.flip(src) if (mosaic and jb["flip"]) else src
        canvas = R.paste(np.full((H, W, 3), 128, np.uint8), R.resize_cubic(pic, (jb["nw"], jb["nh"])), jb["dx"], jb["dy"])
        if not mosaic and jb["flip"]:
            canvas = R.flip(canvas)
        x0, y0, x1, y1 = jb["rect"]
        out[y0:y1, x0:x1] = canvas[y0:y1, x0:x1]
    return out


def regroup(rows, batch, max_boxes):
    """compact rows (N, 6) [image, cls, cx, cy, w, h] -> what cvx_aug_boxes_padded writes: labels (batch, max_boxes, 5) with the first
    max_boxes rows of each image in order and zeros after them, counts (batch,) int32 = min(kept, max_boxes), overflow (0 | 1)"""
    rows = np.asarray(rows, F).reshape(-1, 6)
    labels, counts, overflow = np.zeros((batch, max_boxes, 5), F), np.zeros(batch, np.int32), 0
    for b in range(batch):
        mine = rows[rows[:, 0] == b][:, 1:]
        overflow |= int(len(mine) > max_boxes)
        counts[b] = min(len(mine), max_boxes)
        labels[b, :counts[b]] = mine[:counts[b]]
    return labels, counts, overflow


def per_image_rows(rows, batch):
    """compact rows -> per image the (n_i, 6) label arrays the reference's collate functions receive (column 0 is not read by them)"""
    rows = np.asarray(rows, F).reshape(-1, 6)
    return [rows[rows[:, 0] == b] for b in range(batch)]


# ---- tests/golden/aug_val_ref.npz ----
def load_val_cases(g):
    """fixture -> (H, W, cases); each case with ``job`` in the form draw_params returns, ``boxes``, ``labels``, ``image`` (or None), ``picture``"""
    H, W = (int(v) for v in g["input_shape"])
    cases = []
    for i in range(int(g["n_cases"])):
        c = {k: g[f"c{i}_{k}"] for k in ("sizes", "src_seeds", "boxes", "box_start", "params", "labels")}
        c["image"] = g[f"c{i}_image"] if i in g["image_cases"] else None
        (ih, iw), p = (int(v) for v in c["sizes"][0]), [int(v) for v in c["params"][0]]
        c["job"] = dict(ih=ih, iw=iw, nh=p[0], nw=p[1], dx=p[2], dy=p[3], flip=p[4], quad=p[5], rect=(0, 0, W, H))
        c["picture"] = R.synth_picture(ih, iw, int(c["src_seeds"][0]))
        cases.append(c)
    return H, W, cases
