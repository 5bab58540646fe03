"""The reference's ``detect`` (``utils/detector.py``): the most confident GroundingDINO box for one word on the image that goes to Segment-Anything.

``grounding_dino_model`` is a dict ``{"model": GroundingDinoForObjectDetection, "processor": callable}`` — the pattern of ``sam_model_dict``.  The model
is the caller's ``transformers`` model; with ``GroundingDinoVisionFront.attach(model)`` its Swin backbone and projection levels run on the native
kernels, everything after them as ``transformers`` code.  Nothing here attaches on its own.

``GroundingDinoDetector.from_hf(model, dtype)`` is the whole forward without ``transformers`` between the parts (vision front -> level embeddings and
flattening -> fusion encoder -> query selection, decoder and heads, in the storage dtype throughout; only the caller's BERT ``text_backbone`` stays
``transformers`` code) and goes where the model goes: ``{"model": detector, "processor": ...}``.
"""
from collections import OrderedDict

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


def detect_many(grounding_dino_model, words, images, box_threshold=BOX_THRESHOLD):
    """``detect`` for a list: ONE processor call and ONE forward for ``words[i]`` on ``images[i]`` -> the list of (xyxy, ok) that ``detect`` returns one
    by one.  The captions are padded to one length by the processor; the model masks the padding.  The images are meant to be of one size (the
    character loop's are): images the processor has to pad to a common canvas see that canvas, which a forward of their own would not."""
    model, processor = grounding_dino_model["model"], grounding_dino_model["processor"]
    words, images = list(words), list(images)
    if len(words) != len(images):
        raise ValueError(f"detect_many: {len(words)} words for {len(images)} images")
    if not words:
        return []
    captions = [caption_of([w] if isinstance(w, str) else list(w)) for w in words]
    inputs = processor(images=images, text=captions, return_tensors="pt", padding=True)
    p0 = next(iter(model.parameters()), None) if hasattr(model, "parameters") else None
    if p0 is not None:
        inputs = {k: (v.to(device=p0.device, dtype=p0.dtype) if torch.is_tensor(v) and torch.is_floating_point(v)
                      else v.to(p0.device) if torch.is_tensor(v) else v) for k, v in dict(inputs).items()}
    with torch.no_grad():
        out = model(**inputs)
    logits, boxes = out.logits.float().cpu(), out.pred_boxes.float().cpu()          # one copy for the whole list
    return [select_box(logits[i], boxes[i], *_image_size(images[i]), box_threshold) for i in range(len(words))]


class GroundingDinoDetector:
    """``GroundingDinoForObjectDetection.forward`` for inference on the native parts.  Called with the processor's keyword arguments it returns an object
    with ``.logits`` fp32 [B, Q, max_text_len] and ``.pred_boxes`` fp32 [B, Q, 4] (and ``.topk_proposals``).  It has no ``parameters()``: ``detect`` leaves
    the processor's tensors where they are, and CPU ``input_ids`` are what the caption cache keys on.

    CAPTION CACHE: the text states after ``text_projection`` (with the masks and position ids made from the ids) are kept per caption in an LRU cache of
    ``cache_size`` entries, keyed by the bytes of ``input_ids``, ``attention_mask`` and ``token_type_ids``.  It is used only when those arrive as CPU
    tensors (a processor with ``return_tensors="pt"`` delivers them so): reading device ids would synchronise.  A repeated word costs no BERT run."""

    def __init__(self, config, front, encoder, head, text_backbone, text_projection, level_embed, cache_size=32):
        self.config, self.front, self.encoder, self.head = config, front, encoder, head
        self.text_backbone = text_backbone
        self.device, self.dtype = head.device, head.dtype
        self.text_w = text_projection[0].detach().to(device=self.device, dtype=self.dtype).contiguous()
        self.text_b = text_projection[1].detach().to(device=self.device, dtype=self.dtype).contiguous()
        self.level_embed = level_embed.detach().to(device=self.device, dtype=self.dtype).contiguous()
        self.max_text_len = int(config.max_text_len)
        self.cache_size = int(cache_size)
        self._captions = OrderedDict()
        self._ones, self._geometry = {}, {}
        self.cache_hits = self.cache_misses = 0

    @classmethod
    def from_hf(cls, hf_model, dtype=torch.bfloat16, device=None, cache_size=32):
        """from a ``transformers`` ``GroundingDinoForObjectDetection`` (its weights are copied; its ``text_backbone`` module is kept and called as it is)"""
        from .grounding_dino import GroundingDinoVisionFront
        from .grounding_dino_decoder import GroundingDinoDecoderHead
        from .grounding_dino_encoder import GroundingDinoFusionEncoder
        if not hasattr(hf_model, "model") or not hasattr(hf_model, "bbox_embed"):
            raise TypeError("GroundingDinoDetector.from_hf: a transformers GroundingDinoForObjectDetection expected")
        core, config = hf_model.model, hf_model.config
        if device is None:
            device = next(iter(core.text_backbone.parameters())).device
        sd = hf_model.state_dict()
        return cls(config, GroundingDinoVisionFront.from_state_dict(config, sd, device, dtype),
                   GroundingDinoFusionEncoder.from_state_dict(config, sd, device, dtype),
                   GroundingDinoDecoderHead.from_state_dict(config, sd, device, dtype), core.text_backbone,
                   (core.text_projection.weight, core.text_projection.bias), core.level_embed, cache_size)

    # ---- text --------------------------------------------------------------------------------------------------------------------------------------
    def _encode_text(self, input_ids, attention_mask, token_type_ids):
        """the text lines of ``GroundingDinoModel.forward`` -> (text states [B, Lt, d] storage dtype, token mask bool, self-attention masks bool (True =
        may attend), position ids), all on the device"""
        from transformers.models.grounding_dino.modeling_grounding_dino import generate_masks_with_special_tokens_and_transfer_map
        from . import ops
        allowed, position_ids = generate_masks_with_special_tokens_and_transfer_map(input_ids)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        token_mask = attention_mask.bool()
        T = self.max_text_len
        if allowed.shape[1] > T:
            allowed, position_ids = allowed[:, :T, :T], position_ids[:, :T]
            input_ids, token_type_ids, token_mask = input_ids[:, :T], token_type_ids[:, :T], token_mask[:, :T]
        dev = self.device
        input_ids, token_type_ids, token_mask, allowed, position_ids = (t.to(dev) for t in (input_ids, token_type_ids, token_mask, allowed, position_ids))
        with torch.no_grad():
            feats = self.text_backbone(input_ids, allowed[:, None], token_type_ids, position_ids, return_dict=True).last_hidden_state
            B, Lt, C = feats.shape
            text = ops.linear(feats.to(self.dtype).reshape(B * Lt, C).contiguous(), self.text_w, self.text_b).view(B, Lt, -1)
        return text, token_mask, allowed, position_ids

    def text_states(self, input_ids, attention_mask=None, token_type_ids=None):
        tensors = [t for t in (input_ids, attention_mask, token_type_ids) if t is not None]
        if self.cache_size <= 0 or any(t.device.type != "cpu" for t in tensors):
            return self._encode_text(input_ids, attention_mask, token_type_ids)
        key = (tuple(input_ids.shape),) + tuple(None if t is None else t.contiguous().numpy().tobytes() for t in (input_ids, attention_mask, token_type_ids))
        hit = self._captions.get(key)
        if hit is not None:
            self._captions.move_to_end(key)
            self.cache_hits += 1
            return hit
        self.cache_misses += 1
        hit = self._encode_text(input_ids, attention_mask, token_type_ids)
        self._captions[key] = hit
        while len(self._captions) > self.cache_size:
            self._captions.popitem(last=False)
        return hit

    # ---- what depends on the pixel mask alone ------------------------------------------------------------------------------------------------------
    def _pixel_mask(self, pixel_mask, B, H, W):
        """the mask on the device.  No mask, or a CPU mask without padding (what the processor delivers for images of one size: read on the host, no
        device synchronisation), is ONE persistent all-ones tensor per shape, so that everything cached per mask tensor — the front's level masks and
        position embeddings, ``_mask_geometry``, the encoder's reference points, the head's proposals — is computed once, not per forward."""
        if pixel_mask is None or (pixel_mask.device.type == "cpu" and bool(pixel_mask.all())):
            key = (B, H, W)
            pm = self._ones.get(key)
            if pm is None:
                if len(self._ones) >= 8:
                    self._ones.clear()
                pm = self._ones[key] = torch.ones(key, dtype=torch.long, device=self.device)
            return pm
        return pixel_mask.to(self.device)

    def _mask_geometry(self, pm, feats, pos, maps, shapes):
        """(level position embeddings + level embeddings, flattened [B, Nv, d]; valid bool [B, Nv]; valid ratios fp32 [B, L, 2]), cached per mask TENSOR
        (same object, same ``_version``) as the front caches its masks"""
        key = (id(pm), pm._version, tuple(shapes))
        hit = self._geometry.get(key)
        if hit is None or hit[0] is not pm:
            if len(self._geometry) >= 8:
                self._geometry.clear()
            front, dt = self.front, self.dtype
            masks, pos = [m for _, m in feats], list(pos)
            for level in range(len(feats), len(maps)):                 # the extra level: mask and position embedding of its own size
                masks.append(front.level_mask(pm, maps[level].shape[-2:]))
                pos.append(front.position_embedding(maps[level], masks[-1]).to(dt))
            lvl_pos = torch.cat([p.to(dt).flatten(2).transpose(1, 2) + self.level_embed[i].view(1, 1, -1) for i, p in enumerate(pos)], 1)
            valid = torch.cat([m.flatten(1) for m in masks], 1)
            ratios = torch.stack([torch.stack([m[:, 0, :].sum(1).float() / m.shape[2], m[:, :, 0].sum(1).float() / m.shape[1]], -1) for m in masks], 1)
            hit = (pm, lvl_pos.contiguous(), valid.contiguous(), ratios.contiguous())
            self._geometry[key] = hit
        return hit[1], hit[2], hit[3]

    # ---- forward -----------------------------------------------------------------------------------------------------------------------------------
    def forward(self, pixel_values, input_ids, token_type_ids=None, attention_mask=None, pixel_mask=None, output_attentions=None, **kwargs):
        if output_attentions:
            raise NotImplementedError("GroundingDinoDetector: output_attentions=True (no attention matrix exists in memory)")
        front, dev, dt = self.front, self.device, self.dtype
        text, token_mask, allowed, position_ids = self.text_states(input_ids, attention_mask, token_type_ids)
        with torch.no_grad():
            pv = pixel_values.to(device=dev, dtype=dt)
            B, _, H, W = pv.shape
            pm = self._pixel_mask(pixel_mask, B, H, W)
            feats, pos = front.forward(pv, pm)
            maps = front.project(feats)
            shapes = [tuple(int(v) for v in m.shape[-2:]) for m in maps]
            src = torch.cat([m.flatten(2).transpose(1, 2) for m in maps], 1)
            lvl_pos, valid, ratios = self._mask_geometry(pm, feats, pos, maps, shapes)
            enc = self.encoder.forward(vision_features=src, vision_attention_mask=~valid, vision_position_embedding=lvl_pos, spatial_shapes_list=shapes,
                                       valid_ratios=ratios, text_features=text, text_attention_mask=~token_mask,
                                       text_self_attention_masks=~allowed, text_position_ids=position_ids)
            return self.head.forward(enc.last_hidden_state_vision, valid, enc.last_hidden_state_text, token_mask, shapes, ratios)

    __call__ = forward
