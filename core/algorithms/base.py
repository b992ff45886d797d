"""What the detector wrappers share.  ``Detector``: the two evaluation drivers of the algorithm-class contract, ``evaluate_on_voc`` and
``evaluate_on_coco``, over the model's own ``_evaluation_rows``.  For the two anchor decodes that end in ``cvx_nms_variant`` (YOLOv7,
SSD): ``nms_with_room``, the call that grows its row block until nothing is cut short, and ``NmsDetector``, the map of the kept corner
boxes to the original image."""
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import engine as _engine
from core.utils.boxes import correct_boxes

MAX_DET = 1024          # rows per NMS block cvx_nms_variant is first asked for; a full block is retried with 4x the room, up to ...
MAX_CANDIDATES = 16384  # ... the candidates per block the in-LDS sort holds (the reference's NMS has no limit: only beyond this it raises)


def nms_with_room(y, conf_threshold, nms_threshold, overflow_message, **kw):
    """``cvx_nms_variant`` (vanilla) on ``y`` with room for every kept row, as the reference's unlimited NMS has: MAX_DET rows per block
    first, four times as many while a block comes back full (it may have been cut short), up to MAX_CANDIDATES.  One host read, of the
    counts, per attempt.  Returns (rows, index, counts, the counts on the host); a count of -1 -- more candidates in a block than the
    sort holds -- raises ``CvxError(overflow_message(block))``."""
    max_det = MAX_DET
    while True:
        rows, index, counts = _engine.nms(y, conf_threshold, nms_threshold, max_det=max_det, variant="vanilla", **kw)
        counts_h = counts.cpu()
        found = counts_h.tolist()
        if min(found, default=0) < 0:
            raise L.CvxError(overflow_message(next(i for i, n in enumerate(found) if n < 0)))
        if max(found, default=0) < max_det or max_det >= MAX_CANDIDATES:
            return rows, index, counts, counts_h
        max_det = min(max_det * 4, MAX_CANDIDATES)


class FramePredictor:
    """``detect_frames`` over the class's own ``predict_batch``: what the five algorithm classes share of the video path."""

    def _need_gpu(self, what):
        import torch
        if torch.device(self.device).type != "cuda":
            raise L.CvxError(f"{what} runs on an MI355X only (device {self.device}): there is no CPU path")

    def detect_frames(self, model, frames, batch_size, tiled=None, track=None, tta=None):
        """Generator over any iterable of uint8 HWC RGB device frames: yields the list of drawn frames of each batch of ``batch_size`` (the
        last one may be short).  Each batch is one ``predict_batch(..., draw=True, sync=False)``: nothing inside the loop waits on the
        host, so the caller synchronises (or reads a frame) when it needs the pixels.  ``tiled``: a dict of ``predict_tiled`` keywords
        (the four detectors) -- each batch is then one ``predict_tiled(..., draw=True, sync=False, **tiled)``.  ``track``: a
        ``track.Tracker``, or a dict of its parameters from which one is created for the generator's lifetime (the four detectors) -- every
        batch goes through it in order, and the frames are painted with the track ids (``cvx_draw_tracks``); composes with ``tiled``.
        ``tta``: a ``det_tta.DetTTA`` (the four detectors) -- every batch is predicted on its views and fused, ``predict_batch(...,
        tta=tta)``; composes with ``track``, and is refused together with ``tiled``: augmented tiles are not built."""
        if track is not None and not isinstance(self, Detector):
            raise L.CvxError(f"{type(self).__name__} has no detections to track")
        if tta is not None and not isinstance(self, Detector):
            raise L.CvxError(f"{type(self).__name__} has no detections to augment")
        if tta is not None and tiled is not None:
            raise L.CvxError("detect_frames: tta= together with tiled= is not built (augmentation of tiles); pass one of them")
        self._need_gpu("detect_frames")
        if int(batch_size) <= 0:
            raise ValueError("batch_size is positive")
        more = {}
        if track is not None:
            from computervision.pytorch_amd.track import Tracker
            more["tracker"] = track if isinstance(track, Tracker) else Tracker(self.device, **dict(track))
        if tiled is None:
            if tta is not None:
                more["tta"] = tta

            def predict(model, batch, draw, sync):
                return self.predict_batch(model, batch, draw=draw, sync=sync, **more)
        else:
            if not hasattr(self, "predict_tiled"):
                raise L.CvxError(f"{type(self).__name__} has no tiled prediction")
            tiled = dict(tiled)
            if {"draw", "sync"} & set(tiled):
                raise ValueError("detect_frames draws and does not wait: tiled= takes neither draw nor sync")

            def predict(model, batch, draw, sync):
                return self.predict_tiled(model, batch, draw=draw, sync=sync, **tiled, **more)

        def batches():
            batch = []
            for frame in frames:
                batch.append(frame)
                if len(batch) == int(batch_size):
                    predict(model, batch, draw=True, sync=False)
                    yield batch
                    batch = []
            if batch:
                predict(model, batch, draw=True, sync=False)
                yield batch

        return batches()

    def evaluate_tracking(self, model, sequence, out_root, tracker=None, batch_size=8, tiled=None):
        """Scores the tracker on a sequence with ground-truth identities (the four detectors): ``sequence`` is an iterable of ``(frame, gt)``
        in time order, frame a uint8 HWC RGB device tensor and gt (n <= 1024, 6) float32 ``[x1, y1, x2, y2, cls, identity]`` in the
        frame's pixels, on the device.  Every batch of ``batch_size`` frames is one ``predict_batch(..., tracker=, sync=False)`` -- or, with
        ``tiled`` (a dict of ``predict_tiled`` keywords), one ``predict_tiled`` -- and one ``cvx_mot_frames`` launch
        (``track_eval.TrackingEvaluator``, default parameters); nothing inside the loop waits on the host.  ``tracker``: a
        ``track.Tracker``, a dict of its parameters, or None for the defaults.  One host read at the end: writes
        ``out_root/results/tracking.txt`` and returns ``TrackingEvaluator.get_results()``."""
        if not isinstance(self, Detector):
            raise L.CvxError(f"{type(self).__name__} has no detections to track")
        self._need_gpu("evaluate_tracking")
        if int(batch_size) <= 0:
            raise ValueError("batch_size is positive")
        import os

        import torch
        from computervision.pytorch_amd.track import Tracker
        from computervision.pytorch_amd.track_eval import TrackingEvaluator
        if not isinstance(tracker, Tracker):
            tracker = Tracker(self.device, **dict(tracker or {}))
        if tiled is not None and {"draw", "sync", "tracker"} & set(tiled):
            raise ValueError("evaluate_tracking neither draws nor waits and brings its tracker: tiled= takes none of draw, sync, tracker")
        evaluator = TrackingEvaluator(self.device)

        def flush(frames, truths):
            if tiled is None:
                rows, counts, ids = self.predict_batch(model, frames, sync=False, tracker=tracker)
            else:
                rows, counts, ids = self.predict_tiled(model, frames, sync=False, tracker=tracker, **dict(tiled))
            gt = torch.zeros(len(frames), max(1, max(int(t.shape[0]) for t in truths)), 6, dtype=torch.float32, device=rows.device)
            for b, t in enumerate(truths):
                gt[b, :t.shape[0]] = t
            gt_counts = torch.tensor([int(t.shape[0]) for t in truths], dtype=torch.int32).to(rows.device, non_blocking=True)
            evaluator.add_frames(rows, counts, ids, gt, gt_counts)

        frames, truths = [], []
        for frame, gt in sequence:
            if not (torch.is_tensor(gt) and gt.dim() == 2 and gt.shape[1] == 6 and gt.dtype == torch.float32 and gt.is_cuda):
                raise ValueError("evaluate_tracking: gt is (n, 6) float32 [x1, y1, x2, y2, cls, identity] on the device")
            frames.append(frame)
            truths.append(gt)
            if len(frames) == int(batch_size):
                flush(frames, truths)
                frames, truths = [], []
        if frames:
            flush(frames, truths)
        results = evaluator.get_results()
        evaluator.write_report(os.path.join(out_root, "results", "tracking.txt"))
        return results


class Detector(FramePredictor):
    """Needs ``num_classes``, ``device``, ``eval_max_det`` (the most rows per image ``_evaluation_rows`` returns) and
    ``_evaluation_rows(model) -> rows_of(images, meta, conf_threshold=0.001) -> (rows, counts, box map or None)``."""

    def _predict_input(self):
        """(network input (H, W), letterbox) of ``predict``'s own preprocessing"""
        size = self.input_image_size if hasattr(self, "input_image_size") else self.input_size
        return (int(size[0]), int(size[1])), bool(self.letterbox_image)

    def _box_map_terms(self, image_hw, input_hw):
        """float64 (px, py, gx, gy) of the affine map this class's tail reports its boxes through, ``x_rep = (x_net - px) * gx``, for
        original sizes ``image_hw`` (B, 2) on the device: the arithmetic of ``det_eval.letterbox_box_map`` / ``correct_boxes_device``,
        plain stretching when the class does not letterbox.  ``det_tta.DetTTA`` builds its view maps from it."""
        from computervision.pytorch_amd import det_tta
        return det_tta.box_map_terms(image_hw, input_hw, bool(self.letterbox_image))

    def _augmented(self, model, tta, max_det=None):
        """``_evaluation_rows(model)``, behind ``tta`` when one is given"""
        rows_of = self._evaluation_rows(model)
        if tta is None:
            return rows_of
        from computervision.pytorch_amd.det_tta import DetTTA
        if not isinstance(tta, DetTTA):
            raise ValueError(f"tta: a det_tta.DetTTA or None, got {type(tta).__name__}")
        return tta.wrap(self, rows_of, max_det)

    def _tracked(self, tracker, frames, batch, rows, counts, overflow, draw, sync):
        """The end of ``predict_batch`` / ``predict_tiled`` with a tracker: ids, the tracks painted, the return with its third element"""
        from computervision.pytorch_amd import render
        ids = tracker.update(rows, counts)
        if draw:
            render.draw_tracks(frames, rows, ids, counts, batch=batch)
        if sync:
            return render.read_detections(rows, counts, overflow, ids)
        return rows, counts, ids

    def predict_batch(self, model, frames, conf_threshold=None, draw=False, sync=True, tracker=None, tta=None):
        """``predict`` for a batch, on the device: ``frames`` is a list of uint8 HWC RGB device tensors of any sizes.  One launch builds the
        network batch (``cvx_letterbox_batch_u8_to_nchw`` when ``cfg.decode.letterbox_image``, else the bicubic stretch through
        ``cvx_aug_images_plain`` jobs -- the host ``INTER_CUBIC`` resize of ``predict``), one forward, the class's own decode + NMS tail
        (``_evaluation_rows`` at ``conf_threshold``, default the configured one) and ``cvx_det_to_image``.  ``draw=True`` paints the
        detections into the frames, in place (``cvx_draw_detections``).  Returns ``(rows (B, K, 6) [x1, y1, x2, y2, score, cls] in
        original-image pixels, counts (B) int32)`` on the device; with ``sync=True`` one host read turns them into a list of ``(boxes,
        scores, classes)`` numpy triples in ``decode_box``'s format (and raises ``CvxError`` if an image overflowed the NMS).
        ``tracker``: a ``track.Tracker`` -- the frames are consecutive frames of its stream 0, the rows get track ids after
        ``cvx_det_to_image`` (``cvx_track_update``, no host read), ``draw`` paints them with ``cvx_draw_tracks``, and the return gains a
        third element: ``(rows, counts, ids (B, K) int32)``, or with ``sync=True`` ``(boxes, scores, classes, ids)`` per frame, a row
        without a track with -1.  Without a tracker nothing changes.
        ``tta``: a ``det_tta.DetTTA`` -- the batch runs once per view (the picture at a few zooms and mirrored, every view at the network's
        own size: one ``cvx_det_tta_inputs`` launch) and one ``cvx_det_fuse_views`` launch fuses the views' rows per frame; the rows are
        ``(B, tta.max_det, 6)``.  Drawing, ``sync`` and the tracker see the fused rows.  With None nothing changes."""
        from computervision.pytorch_amd import render
        self._need_gpu("predict_batch")
        frames = list(frames)
        input_hw, letterbox = self._predict_input()
        batch = render.FrameBatch(frames, input_hw, letterbox)
        model.eval()
        conf = self.conf_threshold if conf_threshold is None else conf_threshold
        rows, counts, box_map = self._augmented(model, tta)(batch.network_input(), {"image_hw": batch.image_hw}, conf)
        rows, counts, overflow = render.det_to_image(rows, counts, box_map)
        if tracker is not None:
            return self._tracked(tracker, frames, batch, rows, counts, overflow, draw, sync)
        if draw:
            render.draw_detections(frames, rows, counts, batch=batch)
        if sync:
            return render.read_detections(rows, counts, overflow)
        return rows, counts

    def predict_tiled(self, model, frames, overlap=0.2, full_frame=True, match="ios", match_threshold=0.5, class_agnostic=False, max_det=300,
                      conf_threshold=None, batch_size=32, draw=False, sync=True, tracker=None):
        """``predict_batch`` for frames much larger than the network input, where shrinking the whole picture loses the small objects: every
        frame is cut into tiles of the network's input size that overlap by ``overlap`` (``render.tile_grid``; no resampling, zoom 1), with
        ``full_frame`` one more slot per frame holds the whole picture as ``predict_batch`` would feed it, and one ``cvx_tiles_u8_to_nchw``
        launch builds all slots.  The slots run through the class's own tail (``_evaluation_rows`` at ``conf_threshold``) in chunks of
        ``batch_size`` and through ``cvx_det_to_image``; the chunks are padded to one row block on the device, and one
        ``cvx_det_merge_tiles`` launch moves every row to frame coordinates and suppresses the duplicates across tile borders (``match``:
        ``"ios"`` intersection over the smaller box, or ``"iou"``; above ``match_threshold``; inside a class unless ``class_agnostic``;
        at most ``max_det`` rows per frame).  ``draw`` and ``sync`` as in ``predict_batch``: returns ``(rows (frames, max_det, 6), counts
        (frames) int32)`` on the device, or with ``sync=True`` the list of ``(boxes, scores, classes)`` triples from one host read, which
        raises ``CvxError`` when a slot overflowed its NMS or a frame has more than 8192 candidates.  ``tracker`` as in ``predict_batch``:
        the ids are computed on the merged rows."""
        import torch
        from computervision.pytorch_amd import render
        self._need_gpu("predict_tiled")
        if int(batch_size) <= 0:
            raise ValueError("batch_size is positive")
        frames = list(frames)
        input_hw, letterbox = self._predict_input()
        batch = render.TileBatch(frames, input_hw, overlap, full_frame, letterbox)
        model.eval()
        conf = self.conf_threshold if conf_threshold is None else conf_threshold
        rows_of = self._evaluation_rows(model)
        x = batch.network_input()
        parts, overflow = [], None
        for c0 in range(0, batch.slots, int(batch_size)):
            c1 = min(c0 + int(batch_size), batch.slots)
            rows, counts, box_map = rows_of(x[c0:c1], {"image_hw": batch.image_hw[c0:c1]}, conf)
            rows, counts, overflow = render.det_to_image(rows, counts, box_map, overflow)
            parts.append((c0, c1, rows, counts))
        K = max(int(p[2].shape[1]) for p in parts)              # the tails' row blocks may differ in size: one block, the rest zero
        slot_rows = torch.zeros(batch.slots, K, 6, dtype=torch.float32, device=batch.device)
        for c0, c1, rows, _ in parts:
            slot_rows[c0:c1, :rows.shape[1]] = rows
        slot_counts = torch.cat([p[3] for p in parts])
        rows, counts, _, overflow = render.merge_tiles(slot_rows, slot_counts, batch.slot_map, batch.frame_hw, match, match_threshold, class_agnostic,
                                                       max_det, overflow)
        if tracker is not None:
            return self._tracked(tracker, frames, batch, rows, counts, overflow, draw, sync)
        if draw:
            render.draw_detections(frames, rows, counts, batch=batch)
        if sync:
            return render.read_detections(rows, counts, overflow)
        return rows, counts

    def evaluate_on_voc(self, model, map_out_root, subset="val", dataloader=None, capacity=None, coco_metric=False, tta=None, diagnostics=None):
        """The reference's ``evaluate_on_voc``: VOC mAP (``get_map`` at IoU 0.5) of ``model`` at ``conf_threshold=0.001``, written to
        ``map_out_root/results/results.txt``.  Reading VOC from disk is outside the hot path: ``dataloader`` yields ``(images, meta)`` with
        images (B, 3, H, W) already through the validation transform and meta = dict(image_hw (B, 2) original sizes, gt (B, G, 6) int32
        [cls, l, t, r, b, difficult], gt_counts (B) int32), all on the device, THE IMAGES IN SORTED-ID ORDER (the reference's
        ``dr_files_list.sort()`` decides equal scores).
        Per batch: the model's ``_evaluation_rows`` (its docstring says what that launches and reads) and one ``cvx_det_match`` launch.
        An image without detections contributes none (the reference writes one all-zero line of class 0 for it, YOLOv8's writes
        nothing).  Returns ``DetectionEvaluator.results()``.  No plots.
        ``coco_metric=True`` adds the COCO metric ``get_coco_map`` ends the reference's method with, from the same pass: the ``"coco"``
        entry of the result.
        ``tta``: a ``det_tta.DetTTA`` -- every batch is evaluated on its views and fused (``DetTTA.wrap`` around ``_evaluation_rows``, at
        most ``min(eval_max_det, 8192)`` rows per image); everything behind the rows is unchanged.
        ``diagnostics``: a ``det_diag.DetDiagnostics`` -- the same rows feed one ``cvx_det_confusion`` launch per batch; the confusion
        matrix, the confidence curves with the recommended ``conf_threshold`` and the log-average miss rates are the ``"diagnostics"``
        entry of the result and three files beside ``results.txt``.  None: nothing of it is allocated or launched."""
        if subset not in ("val", "test"):
            raise ValueError(f"sub_set must be one of 'test' and 'val', but got {subset}")
        if dataloader is None:
            raise L.CvxError("evaluate_on_voc reads no dataset from disk: pass dataloader= yielding (images, dict(image_hw, gt, gt_counts)) on the "
                             "device over the VOC-" + subset + " pictures in sorted-id order")
        from computervision.pytorch_amd import det_eval
        from configs.dataset_cfg import VOC_CFG
        model.eval()
        return det_eval.evaluate_detector(self._augmented(model, tta, min(self.eval_max_det, 8192)), dataloader, self.num_classes, self.device,
                                          map_out_root, det_eval.class_names(VOC_CFG, self.num_classes), self.eval_max_det, capacity, coco_metric,
                                          diagnostics)

    def evaluate_on_coco(self, model, map_out_root, subset="val", dataloader=None, capacity=None, tta=None):
        """The reference's ``evaluate_on_coco``: the COCO metric (``COCOeval`` on boxes) of ``model`` at ``conf_threshold=0.001``, boxes and
        scores unrounded.  Reading COCO from disk, category ids and the annotation JSON are outside the hot path: ``dataloader`` yields
        ``(images, meta)`` with images (B, 3, H, W) already through the validation transform and meta = dict(image_hw (B, 2) original sizes,
        gt_coco (B, G, 7) float64 [class index, x, y, w, h, area, iscrowd], gt_counts (B) int32), all on the device, THE IMAGES IN
        SORTED-ID ORDER.
        The rows come from the pass ``evaluate_on_voc`` runs; per batch one ``cvx_coco_match`` launch, and the host reads once, at the end.
        Writes the twelve summary lines to ``map_out_root/coco_results.txt``, prints them and returns ``CocoEvaluator.results()``.
        ``tta`` as in ``evaluate_on_voc``."""
        from computervision.pytorch_amd import coco_eval
        coco_eval.check_coco_arguments(subset, dataloader)
        model.eval()
        return coco_eval.evaluate_detector_coco(self._augmented(model, tta, min(self.eval_max_det, 8192)), dataloader, self.num_classes, map_out_root,
                                                self.eval_max_det, capacity)


class NmsDetector(Detector):
    """Needs ``input_image_size`` and ``letterbox_image`` besides."""
    eval_max_det = MAX_CANDIDATES

    def _correct_boxes(self, box_xy, box_wh, input_shape, image_shape):
        return correct_boxes(box_xy, box_wh, input_shape, image_shape, self.letterbox_image)

    def _to_image(self, det, image_h, image_w):
        """Rows that begin with normalised corners [x1, y1, x2, y2] (numpy, changed in place) -> the same rows in original-image pixels"""
        xy, wh = (det[:, 0:2] + det[:, 2:4]) / 2, det[:, 2:4] - det[:, 0:2]
        det[:, :4] = self._correct_boxes(xy, wh, self.input_image_size, [image_h, image_w])
        return det
