"""Video detection on the device (the reference's scripts/detect.py:detect_video): frames are decoded on the host, moved to the GPU,
predicted and drawn batch by batch by the algorithm's ``predict_batch`` and encoded again.  No frame goes through a temporary JPEG file,
and nothing between decode and encode waits on the host inside a batch.  Decode and encode need OpenCV, imported lazily; everything
between them does not."""
import torch

from computervision.pytorch_amd._lib import CvxError


def detect_frames(algorithm, model, frames, batch_size, tiled=None):
    """Generator over any iterable of uint8 HWC RGB device frames: yields the drawn frames (the same tensors, painted in place) as one list
    per batch of ``batch_size``.  ``algorithm`` is one of the five algorithm objects; each batch is its ``predict_batch(..., draw=True,
    sync=False)``, so the loop never waits on the host.  ``tiled``: a dict of ``predict_tiled`` keywords for footage much larger than the
    network input (the four detectors): each batch is then cut into tiles, detected and merged on the device."""
    return algorithm.detect_frames(model, frames, batch_size, tiled=tiled)


def detect_video(model, src_video_path, dst_video_path, decode_fn, batch_size=8, tiled=None):
    """The reference's signature: ``decode_fn`` is the bound ``predict`` of an algorithm object (as the reference passes it) or the algorithm
    object itself.  Reads ``src_video_path`` frame by frame, draws the predictions on the device and writes ``dst_video_path`` with the
    source's frame rate and size.  ``tiled`` as in ``detect_frames``."""
    algorithm = getattr(decode_fn, "__self__", decode_fn)
    if not hasattr(algorithm, "predict_batch"):
        raise CvxError("detect_video: decode_fn is an algorithm object or its bound predict method")
    try:
        import cv2
    except ImportError as e:  # pragma: no cover
        raise ImportError("detect_video needs opencv-python to decode and encode video; detect_frames takes frames that are already on the "
                          "device") from e
    capture = cv2.VideoCapture(src_video_path)
    if not capture.isOpened():
        raise FileNotFoundError(src_video_path)
    fps = capture.get(cv2.CAP_PROP_FPS)
    size = (int(capture.get(cv2.CAP_PROP_FRAME_WIDTH)), int(capture.get(cv2.CAP_PROP_FRAME_HEIGHT)))
    writer = cv2.VideoWriter(dst_video_path, cv2.VideoWriter_fourcc(*"mp4v"), fps, size)
    device = torch.device(algorithm.device)

    def decoded():
        while True:
            ok, bgr = capture.read()
            if not ok:
                return
            yield torch.from_numpy(cv2.cvtColor(bgr, cv2.COLOR_BGR2RGB)).to(device, non_blocking=True)

    try:
        for batch in detect_frames(algorithm, model, decoded(), batch_size, tiled=tiled):
            for frame in batch:                                   # the host read of a finished batch: the only wait
                writer.write(cv2.cvtColor(frame.cpu().numpy(), cv2.COLOR_RGB2BGR))
    finally:
        capture.release()
        writer.release()
