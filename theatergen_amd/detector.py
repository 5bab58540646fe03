"""The reference's ``detect`` (``utils/detector.py``): the most confident GroundingDINO box for one word on the image that goes to Segment-Anything.

``grounding_dino_model`` is a dict ``{"model": GroundingDinoForObjectDetection, "processor": callable}`` — the pattern of ``sam_model_dict``.  The model
is the caller's ``transformers`` model; with ``GroundingDinoVisionFront.attach(model)`` its Swin backbone and projection levels run on the native
kernels, everything after them as ``transformers`` code.  Nothing here attaches on its own.
"""
import numpy as np
import torch

BOX_THRESHOLD = 0.3
TEXT_THRESHOLD = 0.25


def caption_of(classes):
    """GroundingDINO's ``predict_with_classes`` caption: the lower-cased classes joined by ``". "``"""
    return ". ".join(str(c).lower().strip() for c in classes)


def _image_size(image):
    if hasattr(image, "size") and not hasattr(image, "shape"):                  # PIL: (width, height)
        w, h = image.size
        return int(h), int(w)
    shape = tuple(image.shape)
    if len(shape) == 3 and shape[0] in (1, 3) and shape[-1] not in (1, 3):      # CHW
        return int(shape[1]), int(shape[2])
    return int(shape[0]), int(shape[1])


def select_box(logits, pred_boxes, height, width, box_threshold=BOX_THRESHOLD):
    """logits [queries, tokens] (before the sigmoid), pred_boxes [queries, 4] normalised cxcywh -> (xyxy in source-image pixels, ok).
    A query counts if the maximum over tokens of its sigmoid logit EXCEEDS ``box_threshold``; that maximum is its confidence."""
    conf = torch.sigmoid(torch.as_tensor(logits).float()).max(dim=-1).values
    if conf.numel() == 0 or not bool((conf > box_threshold).any()):
        return np.zeros(4, np.float32), False
    best = int(torch.argmax(conf))
    cx, cy, w, h = [float(v) for v in torch.as_tensor(pred_boxes)[best].float().cpu()]
    cx, w = cx * width, w * width
    cy, h = cy * height, h * height
    return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], np.float32), True


def detect(grounding_dino_model, word, sam_input_image, box_threshold=BOX_THRESHOLD):
    """-> (xyxy of the most confident box in pixels of ``sam_input_image``, ok): the reference's signature and return.  ``ok`` is False when no query
    is over the box threshold (0.3).  The reference also passes a text threshold (0.25); it only names the phrases of a box, which the reference
    discards, so it is not used here."""
    model, processor = grounding_dino_model["model"], grounding_dino_model["processor"]
    classes = [word] if isinstance(word, str) else list(word)
    inputs = processor(images=sam_input_image, text=caption_of(classes), return_tensors="pt")
    p0 = next(iter(model.parameters()), None) if hasattr(model, "parameters") else None
    if p0 is not None:
        inputs = {k: (v.to(device=p0.device, dtype=p0.dtype) if torch.is_tensor(v) and torch.is_floating_point(v)
                      else v.to(p0.device) if torch.is_tensor(v) else v) for k, v in dict(inputs).items()}
    with torch.no_grad():
        out = model(**inputs)
    height, width = _image_size(sam_input_image)
    return select_box(out.logits[0], out.pred_boxes[0], height, width, box_threshold)
