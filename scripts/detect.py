"""Video detection on the device (the reference's scripts/detect.py:detect_video): frames are decoded on the host, moved to the GPU,
predicted and drawn batch by batch by the algorithm's ``predict_batch`` and encoded again.  No frame goes through a temporary JPEG file,
and nothing between decode and encode waits on the host inside a batch.  Decode and encode need OpenCV, imported lazily; everything
between them does not."""
import torch

from computervision.pytorch_amd._lib import CvxError


def detect_frames(algorithm, model, frames, batch_size, tiled=None, track=None, tta=None):
    """Generator over any iterable of uint8 HWC RGB device frames: yields the drawn frames (the same tensors, painted in place) as one list
    per batch of ``batch_size``.  ``algorithm`` is one of the five algorithm objects; each batch is its ``predict_batch(..., draw=True,
    sync=False)``, so the loop never waits on the host.  ``tiled``: a dict of ``predict_tiled`` keywords for footage much larger than the
    network input (the four detectors): each batch is then cut into tiles, detected and merged on the device.  ``track``: a
    ``track.Tracker`` or a dict of its parameters (the four detectors): the detections keep an identity from frame to frame, on the device,
    and are painted with their track ids.  ``tta``: a ``det_tta.DetTTA`` (the four detectors): every batch is predicted at a few zooms and
    mirrored and the views are fused on the device; not together with ``tiled``."""
    return algorithm.detect_frames(model, frames, batch_size, tiled=tiled, track=track, tta=tta)


def segment_frames(algorithm, model, frames, batch_size, regions=None, track=None, **tiled):
    """``detect_frames`` for sliding-window segmentation: ``algorithm`` is the DeepLab algorithm object, each batch is its
    ``segment_tiled(..., draw=True, sync=False, **tiled)`` -- tiles at network size, logits stitched on the device, the class colours
    blended into the frames in place.  ``regions``: a ``seg_regions.SegRegions`` -- the connected regions of the label maps are boxed on
    the device and painted over the overlay; ``track``: a ``track.Tracker`` or a dict of its parameters -- the regions keep an identity
    from frame to frame.  With both None nothing changes."""
    if not hasattr(algorithm, "segment_frames"):
        raise CvxError(f"{type(algorithm).__name__} has no sliding-window segmentation")
    if regions is None and track is None:
        return algorithm.segment_frames(model, frames, batch_size, **tiled)
    return algorithm.segment_frames(model, frames, batch_size, regions=regions, track=track, **tiled)


def _run_video(src_video_path, dst_video_path, device, batches_of):
    """decode -> ``batches_of(frames on the device)`` -> encode, with the source's frame rate and size"""
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

    def decoded():
        while True:
            ok, bgr = capture.read()
            if not ok:
                return
            yield torch.from_numpy(cv2.cvtColor(bgr, cv2.COLOR_BGR2RGB)).to(device, non_blocking=True)

    try:
        for batch in batches_of(decoded()):
            for frame in batch:                                   # the host read of a finished batch: the only wait
                writer.write(cv2.cvtColor(frame.cpu().numpy(), cv2.COLOR_RGB2BGR))
    finally:
        capture.release()
        writer.release()


def detect_video(model, src_video_path, dst_video_path, decode_fn, batch_size=8, tiled=None, track=None, tta=None):
    """The reference's signature: ``decode_fn`` is the bound ``predict`` of an algorithm object (as the reference passes it) or the algorithm
    object itself.  Reads ``src_video_path`` frame by frame, draws the predictions on the device and writes ``dst_video_path`` with the
    source's frame rate and size.  ``tiled``, ``track`` and ``tta`` as in ``detect_frames``."""
    algorithm = getattr(decode_fn, "__self__", decode_fn)
    if not hasattr(algorithm, "predict_batch"):
        raise CvxError("detect_video: decode_fn is an algorithm object or its bound predict method")
    _run_video(src_video_path, dst_video_path, torch.device(algorithm.device),
               lambda frames: detect_frames(algorithm, model, frames, batch_size, tiled=tiled, track=track, tta=tta))


def segment_video(model, src_video_path, dst_video_path, decode_fn, batch_size=2, regions=None, track=None, **tiled):
    """``detect_video`` for full-resolution segmentation: every frame goes through ``segment_tiled`` (``tiled``: its keywords ``overlap``,
    ``weight``, ``bgr``; ``batch_size`` is the frames per call, the slots per forward stay at its default) instead of being stretched to
    the network input.  ``regions`` and ``track`` as in ``segment_frames``."""
    algorithm = getattr(decode_fn, "__self__", decode_fn)
    if not hasattr(algorithm, "segment_frames"):
        raise CvxError("segment_video: decode_fn is the DeepLab algorithm object or its bound predict method")
    _run_video(src_video_path, dst_video_path, torch.device(algorithm.device),
               lambda frames: segment_frames(algorithm, model, frames, batch_size, regions=regions, track=track, **tiled))
