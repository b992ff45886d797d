"""Host-side box bookkeeping after the GPU NMS: normalise to the network input and undo the letterbox.

Follows YOLOv8.decode_box (reference core/algorithms/yolo_v8.py:229-242) and reverse_letter_box_numpy
(reference core/utils/image_process.py:69-97).  A few dozen boxes per image: numpy on the host, as in
the reference.
"""
import numpy as np


def undo_letterbox(rows: np.ndarray, input_hw, image_hw, letterbox: bool = True):
    """rows (k,6) [x1,y1,x2,y2,conf,cls] in network-input pixels -> (boxes (k,4) in original-image pixels, conf, cls)."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 6)
    in_h, in_w = (float(v) for v in input_hw)
    img_h, img_w = (float(v) for v in image_hw)
    conf, cls = rows[:, 4].copy(), rows[:, 5].astype(np.int64)     # the reference's np.int is gone from NumPy >= 1.24
    box = rows[:, :4].copy()
    if letterbox:
        gain = max(img_h / in_h, img_w / in_w)
        pad_top = (in_h - img_h / gain) // 2
        pad_left = (in_w - img_w / gain) // 2
        box[:, 0::2] -= pad_left
        box[:, 1::2] -= pad_top
        box *= gain
    else:
        box[:, 0::2] *= img_w / in_w
        box[:, 1::2] *= img_h / in_h
    return box, conf, cls


def correct_boxes(box_xy, box_wh, input_shape, image_shape, letterbox: bool):
    """yolo_correct_boxes (reference core/utils/image_process.py:161-181), what the YOLOv7 and SSD wrappers end their decode with:
    normalised centres (n, 2) and sizes (n, 2) on the (h, w) network input -> corners (n, 4) in pixels of the (h, w) original image, by
    the letterbox inverse or by plain scaling to the image size."""
    xywh = np.concatenate([box_xy, box_wh], axis=-1)
    if letterbox:
        ih, iw = image_shape
        h, w = input_shape
        scale = max(ih / h, iw / w)
        top, left = (h - ih / scale) // 2, (w - iw / scale) // 2
        cx, cy, bw, bh = xywh[:, 0] * w - left, xywh[:, 1] * h - top, xywh[:, 2] * w, xywh[:, 3] * h
        return np.stack([(cx - bw / 2) * scale, (cy - bh / 2) * scale, (cx + bw / 2) * scale, (cy + bh / 2) * scale], -1)
    out = np.stack([xywh[:, 0] - xywh[:, 2] / 2, xywh[:, 1] - xywh[:, 3] / 2, xywh[:, 0] + xywh[:, 2] / 2, xywh[:, 1] + xywh[:, 3] / 2], -1)
    out[:, ::2] *= image_shape[1]
    out[:, 1::2] *= image_shape[0]
    return out
