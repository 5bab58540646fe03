"""Segment-Anything between the two stages: the SAM image encoder on the native kernels, and the reference's call surface around it
(reference ``models/sam.py``: ``sam`` :26-56, ``select_mask`` :68-112, ``sam_refine_attn`` :126-174).

The encoder (``transformers.SamVisionEncoder``: a ViT at 1024 x 1024, 4096 tokens; ViT-H 32 layers x 1280 channels x 16 heads of 80) is >99 % of
the model and the reference runs it TWICE per character (``sam_refine_attn`` calls ``sam_box_input`` once per target mask shape).  Here
``sam_refine_attn`` computes the embeddings once and serves both shapes; the prompt encoder and mask decoder stay the caller's transformers modules
(``SamModel(image_embeddings=..., input_boxes=...)``) — unless ``sam_model`` is ``theatergen_amd.sam_decoder.SamModel``: then prompt encoder, mask decoder and
the mask post-processing run on the device as well (``_sam_device``: one processor call, one encoder run, one decoder run, one copy back), for one character
(``sam``, ``sam_refine_attn``) or a list of them (``sam_refine_characters``).

Token-major throughout, as ``clip.py``: patch embedding = one GEMM over the unfolded 16 x 16 patches with ``pos_embed`` as the residual operand;
per layer LayerNorm, one Q|K|V^T projection GEMM, ``relpos_tables`` + ``attention_relpos`` (the decomposed relative-position bias added tile by tile,
no [N, N] tensor), proj + residual, LayerNorm, lin1 + exact GELU, lin2 + residual.  Windowed layers: the 64 x 64 grid is zero-padded AFTER layer_norm1
to 70 x 70 and cut into 25 windows of 14 x 14; the padded tokens are zero rows into ``qkv`` (their q, k, v equal the projection's bias), take part in
their window's softmax as real keys, and are dropped by the un-partition before the residual add.  The gather / scatter between image order and
window order is torch indexing (data movement).  Neck: 1 x 1 conv (GEMM), per-pixel channel LayerNorm, 3 x 3 conv, channel LayerNorm, one transpose
to NCHW.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .unet import _Packed
from .weights_pack import pack_conv1x1, pack_conv3x3

SUPPORTED = "image 1024, patch 16 (a 64 x 64 token grid), window 14, head dim 64 or 80, use_abs_pos, use_rel_pos, qkv_bias"


class SamVisionConfig(SimpleNamespace):
    pass


def _config(hidden, layers, heads, global_idx, mlp):
    return SamVisionConfig(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, global_attn_indexes=list(global_idx), mlp_dim=mlp,
                           image_size=1024, patch_size=16, window_size=14, output_channels=256, layer_norm_eps=1e-6, qkv_bias=True,
                           use_abs_pos=True, use_rel_pos=True, num_channels=3)


def sam_vit_h_config():
    """facebook/sam-vit-huge vision tower (the reference's ``models/sam_vit_ckpt``)."""
    return _config(1280, 32, 16, (7, 15, 23, 31), 5120)


def sam_vit_l_config():
    return _config(1024, 24, 16, (5, 11, 17, 23), 4096)


def sam_vit_b_config():
    return _config(768, 12, 12, (2, 5, 8, 11), 3072)


# ---- index maps (host, built once per device) -----------------------------------------------------------------------------------------------
def relative_index(size):
    """[size, size] long: row of a [2 size - 1, d] rel_pos table for (query coordinate, key coordinate) = q - k + size - 1."""
    return torch.arange(size)[:, None] - torch.arange(size)[None, :] + size - 1


def window_gather_index(grid=64, window=14):
    """long [nw * nw * window * window]: for every position of the window-ordered sequence (window row-major, then token row-major inside the window)
    the image token it holds, or ``grid * grid`` for a padded position (the caller appends one zero row there)."""
    nw = (grid + window - 1) // window
    pad = nw * window
    idx = torch.full((pad, pad), grid * grid, dtype=torch.long)
    idx[:grid, :grid] = torch.arange(grid * grid).reshape(grid, grid)
    return idx.reshape(nw, window, nw, window).permute(0, 2, 1, 3).reshape(-1)


def window_scatter_index(grid=64, window=14):
    """long [grid * grid]: where image token i sits in the window-ordered sequence (the un-partition is a gather with this map)."""
    nw = (grid + window - 1) // window
    i = torch.arange(grid * grid)
    r, c = i // grid, i % grid
    return ((r // window) * nw + c // window) * window * window + (r % window) * window + c % window


class _SamLayer(nn.Module):
    def __init__(self, cfg, window):
        super().__init__()
        D, d = cfg.hidden_size, cfg.hidden_size // cfg.num_attention_heads
        self.window = window
        self.size = window if window > 0 else cfg.image_size // cfg.patch_size
        self.layer_norm1 = nn.LayerNorm(D, eps=cfg.layer_norm_eps)
        att = nn.Module()
        att.qkv, att.proj = nn.Linear(D, 3 * D, bias=True), nn.Linear(D, D)
        att.rel_pos_h = nn.Parameter(torch.zeros(2 * self.size - 1, d))
        att.rel_pos_w = nn.Parameter(torch.zeros(2 * self.size - 1, d))
        self.attn = att
        self.layer_norm2 = nn.LayerNorm(D, eps=cfg.layer_norm_eps)
        mlp = nn.Module()
        mlp.lin1, mlp.lin2 = nn.Linear(D, cfg.mlp_dim), nn.Linear(cfg.mlp_dim, D)
        self.mlp = mlp

    def attention(self, y, items, cfg):
        """y [items * S^2, D] (LayerNorm output, image or window order) -> attention output before ``proj``, same order."""
        D, H = cfg.hidden_size, cfg.num_attention_heads
        d, S = D // H, self.size
        L = S * S
        a = self.attn
        ldt = (L + 7) // 8 * 8
        qk = torch.empty((items * L, 2 * D), dtype=y.dtype, device=y.device)
        vt = torch.zeros((items, D, ldt), dtype=y.dtype, device=y.device)
        ops.gemm(y, a.qkv.weight, items * L, 3 * D, D, bias=a.qkv.bias, rows_per_batch=L, out=qk, n_split=2 * D, out_t=vt, ldt=ldt)
        bh, bw = ops.relpos_tables(qk, 2 * D, L * 2 * D, a.rel_pos_h, a.rel_pos_w, items, H, d, S)
        o = torch.empty((items * L, D), dtype=y.dtype, device=y.device)
        return ops.attention_relpos(qk, 2 * D, L * 2 * D, qk[:, D:], 2 * D, L * 2 * D, vt, ldt, D * ldt, items, H, d, S, float(d) ** -0.5, bh, bw,
                                    o, D, L * D)

    def run(self, x, B, cfg, maps):
        D = cfg.hidden_size
        N = (cfg.image_size // cfg.patch_size) ** 2
        y = ops.layernorm(x, self.layer_norm1.weight, self.layer_norm1.bias, cfg.layer_norm_eps)
        if self.window > 0:
            gidx, sidx = maps
            nwin = gidx.numel() // (self.window * self.window)
            yz = torch.cat([y.reshape(B, N, D), torch.zeros((B, 1, D), dtype=y.dtype, device=y.device)], 1)
            yw = yz[:, gidx].reshape(-1, D)                                    # window order, zero rows for the padding
            o = self.attention(yw, B * nwin, cfg)
            o = o.reshape(B, -1, D)[:, sidx].reshape(B * N, D)                 # un-partition: the padded tokens' outputs are dropped
        else:
            o = self.attention(y, B, cfg)
        x = ops.linear(o, self.attn.proj.weight, self.attn.proj.bias, res=x)
        y = ops.layernorm(x, self.layer_norm2.weight, self.layer_norm2.bias, cfg.layer_norm_eps)
        y = ops.linear(y, self.mlp.lin1.weight, self.mlp.lin1.bias, act=ops.ACT_GELU)
        return ops.linear(y, self.mlp.lin2.weight, self.mlp.lin2.bias, res=x)


class SamVisionEncoder(nn.Module):
    """``transformers.SamVisionEncoder`` (same parameter names) on the native kernels; GPU only."""

    def __init__(self, config=None):
        super().__init__()
        cfg = config if config is not None else sam_vit_h_config()
        d = cfg.hidden_size // cfg.num_attention_heads
        bad = []
        if cfg.image_size != 1024:
            bad.append(f"image_size {cfg.image_size}")
        if cfg.patch_size != 16:
            bad.append(f"patch_size {cfg.patch_size}")
        if cfg.window_size != 14:
            bad.append(f"window_size {cfg.window_size}")
        if cfg.hidden_size % cfg.num_attention_heads or d not in (64, 80):
            bad.append(f"head dim {cfg.hidden_size}/{cfg.num_attention_heads}")
        for flag in ("use_abs_pos", "use_rel_pos", "qkv_bias"):
            if not getattr(cfg, flag, True):
                bad.append(f"{flag}=False")
        if bad:
            raise NotImplementedError(f"SamVisionEncoder: {', '.join(bad)} has no kernel; supported: {SUPPORTED}")
        self.config = cfg
        D, g = cfg.hidden_size, cfg.image_size // cfg.patch_size
        self.pos_embed = nn.Parameter(torch.zeros(1, g, g, D))
        pe = nn.Module()
        pe.projection = nn.Conv2d(3, D, cfg.patch_size, stride=cfg.patch_size)
        self.patch_embed = pe
        self.layers = nn.ModuleList([_SamLayer(cfg, 0 if i in cfg.global_attn_indexes else cfg.window_size) for i in range(cfg.num_hidden_layers)])
        neck = nn.Module()
        C = cfg.output_channels
        neck.conv1 = nn.Conv2d(D, C, 1, bias=False)
        neck.layer_norm1 = nn.LayerNorm(C, eps=1e-6)
        neck.conv2 = nn.Conv2d(C, C, 3, padding=1, bias=False)
        neck.layer_norm2 = nn.LayerNorm(C, eps=1e-6)
        self.neck = neck
        self._p = _Packed()
        self._maps = {}
        for p_ in self.parameters():
            p_.requires_grad_(False)

    @property
    def dtype(self):
        return self.pos_embed.dtype

    @property
    def device(self):
        return self.pos_embed.device

    def _window_maps(self, device):
        if device not in self._maps:
            g = self.config.image_size // self.config.patch_size
            self._maps[device] = (window_gather_index(g, self.config.window_size).to(device), window_scatter_index(g, self.config.window_size).to(device))
        return self._maps[device]

    def forward(self, pixel_values, output_hidden_states=False):
        """pixel_values [B, 3, 1024, 1024] -> [B, output_channels, 64, 64] in the model dtype (with ``output_hidden_states``: the pair
        (that, [the [B, 64, 64, hidden] state after every layer]))."""
        if not pixel_values.is_cuda or self.device.type != "cuda":
            raise RuntimeError("theatergen_amd SAM encoder runs on the GPU only (no CPU fallback)")
        cfg, dt = self.config, self.dtype
        B, ch, Hh, Ww = pixel_values.shape
        if ch != 3 or Hh != cfg.image_size or Ww != cfg.image_size:
            raise ValueError(f"SamVisionEncoder: pixel_values {tuple(pixel_values.shape)}, expected [B, 3, {cfg.image_size}, {cfg.image_size}]")
        ps, D = cfg.patch_size, cfg.hidden_size
        g = cfg.image_size // ps
        n, K = g * g, 3 * ps * ps
        wp = self._p.get("patch", [self.patch_embed.projection.weight], lambda: self.patch_embed.projection.weight.detach().reshape(D, K).contiguous())
        pos = self._p.get(("pos", B), [self.pos_embed], lambda: self.pos_embed.detach().reshape(n, D).repeat(B, 1).contiguous())
        patches = pixel_values.to(dt).reshape(B, 3, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * n, K).contiguous()     # unfold = data movement
        x = ops.gemm(patches, wp, B * n, D, K, bias=self.patch_embed.projection.bias, res=pos)
        maps = self._window_maps(pixel_values.device)
        hs = []
        for layer in self.layers:
            x = layer.run(x, B, cfg, maps)
            if output_hidden_states:
                hs.append(x.reshape(B, g, g, D))
        nk, C = self.neck, cfg.output_channels
        w1 = self._p.get("neck1", [nk.conv1.weight], lambda: pack_conv1x1(nk.conv1.weight.detach()))
        # the conv kernels take input channels in multiples of 64: a narrower neck (test configurations; SAM's is 256) gets zero channels appended,
        # in the LayerNorm's output buffer and in the packed weight
        Cp = (C + 63) // 64 * 64
        w2 = self._p.get("neck2", [nk.conv2.weight], lambda: pack_conv3x3(torch.nn.functional.pad(nk.conv2.weight.detach(), (0, 0, 0, 0, 0, Cp - C))))
        y = ops.linear(x, w1)
        yp = torch.empty((B * n, C), dtype=dt, device=x.device) if Cp == C else torch.zeros((B * n, Cp), dtype=dt, device=x.device)
        ops.layernorm(y, nk.layer_norm1.weight, nk.layer_norm1.bias, 1e-6, out=yp[:, :C])
        y = ops.conv3x3(yp, w2, B, g, g, Cp)
        y = ops.layernorm(y, nk.layer_norm2.weight, nk.layer_norm2.bias, 1e-6)
        out = ops.transpose(y, B, n, C).reshape(B, C, g, g)
        return (out, hs) if output_hidden_states else out

    __call__ = forward

    @classmethod
    def from_state_dict(cls, config, state_dict, device="cuda", dtype=torch.bfloat16):
        """``state_dict``: a ``SamVisionEncoder`` state dict, or a whole ``SamModel`` one (keys under ``vision_encoder.`` are taken, the prompt encoder,
        mask decoder and shared embedding are ignored).  A missing or unexpected vision key is a RuntimeError."""
        m = cls(config)
        pre = "vision_encoder."
        if any(k.startswith(pre) for k in state_dict):
            sd = {k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}
        else:
            sd = dict(state_dict)
        missing, unexpected = m.load_state_dict(sd, strict=False)
        if unexpected or missing:
            raise RuntimeError(f"state dict mismatch: missing {missing[:5]}... unexpected {unexpected[:5]}...")
        return m.to(device=device, dtype=dtype)


# ---- the reference's call surface ----------------------------------------------------------------------------------------------------------
def _listify_boxes(input_boxes):
    if input_boxes and isinstance(input_boxes[0], tuple):
        input_boxes = [list(b) for b in input_boxes]
    if input_boxes and input_boxes[0] and isinstance(input_boxes[0][0], tuple):
        input_boxes = [[list(b) for b in item] for item in input_boxes]
    return input_boxes


def sam_image_embeddings(sam_model_dict, image):
    """The encoder half of ``sam``: processor -> our encoder -> [B, 256, 64, 64] in the encoder's dtype."""
    enc, proc = sam_model_dict["sam_encoder"], sam_model_dict["sam_processor"]
    inputs = proc(image, return_tensors="pt")
    with torch.no_grad():
        return enc(inputs["pixel_values"].to(enc.device))


def _on_device_route(sam_model):
    from .sam_decoder import SamModel
    return isinstance(sam_model, SamModel)


def _prompt_array(x, last, what):
    """nested lists / tuples / arrays / CPU tensors -> float64 [B, nb, ..., last]: one image's prompts may come without the image axis"""
    a = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    if a.ndim == 0 or a.shape[-1] != last:
        raise ValueError(f"{what}: last dimension {last} expected, got shape {a.shape}")
    want = 3 if last == 4 else 4
    while a.ndim < want:
        a = a[None]
    if a.ndim != want:
        raise ValueError(f"{what}: shape {a.shape} has too many dimensions")
    return a


def _sam_device(sam_model_dict, images, input_points, input_boxes, target_shapes, image_embeddings=None):
    """The device route behind ``sam`` / ``sam_refine_attn`` / ``sam_refine_characters``: ONE processor call (image resize + normalisation; prompts are
    rescaled here, as the processor does: x * new_w / old_w, y * new_h / old_h in float64), one encoder run unless ``image_embeddings`` come along, one
    decoder run, one ``ops.sam_mask_post`` launch per image and target shape, ONE copy back.
    -> (masks[t][b] bool [nb, m, h_t, w_t] (torch, host), areas[t][b] int64 [nb, m], iou fp32 numpy [B, nb, m])"""
    model, proc = sam_model_dict["sam_model"], sam_model_dict["sam_processor"]
    with torch.no_grad():
        inputs = proc(images, return_tensors="pt")
        pv = inputs["pixel_values"]
        orig = np.asarray(inputs["original_sizes"]).reshape(-1, 2).astype(np.int64)
        resh = np.asarray(inputs["reshaped_input_sizes"]).reshape(-1, 2).astype(np.int64)
        B, S = int(pv.shape[0]), int(pv.shape[-1])
        ratio = np.stack([resh[:, 1] / orig[:, 1], resh[:, 0] / orig[:, 0]], -1)                      # [B, (x, y)]
        kw = {}
        if input_boxes is not None:
            bx = _prompt_array(input_boxes, 4, "input_boxes")
            kw["input_boxes"] = (bx.reshape(bx.shape[0], -1, 2, 2) * ratio[:, None, None, :]).reshape(bx.shape)
        if input_points is not None:
            pts = _prompt_array(input_points, 2, "input_points")
            kw["input_points"] = pts * ratio[:, None, None, :]
            kw["input_labels"] = np.ones(pts.shape[:3], np.int32)
        for k, v in kw.items():
            if v.shape[0] != B:
                raise ValueError(f"{k}: prompts for {v.shape[0]} images, {B} images")
        if image_embeddings is None:
            enc = sam_model_dict.get("sam_encoder") or model.vision_encoder
            image_embeddings = enc(pv.to(model.device))
        out = model(image_embeddings=image_embeddings, **kw)
        dev_masks, dev_areas = [], []
        for shape in target_shapes:
            for b in range(B):
                m, a = ops.sam_mask_post(out.pred_masks[b], S, resh[b], orig[b], shape)
                dev_masks.append(m)
                dev_areas.append(a)
        # one copy back: every result as bytes of one buffer, widest elements first (the host views stay aligned)
        parts = dev_areas + [out.iou_scores] + dev_masks
        flat = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu()
    host, o = [], 0
    for t in parts:
        nbytes = t.numel() * t.element_size()
        host.append(flat[o:o + nbytes].clone().view(t.dtype).reshape(t.shape))
        o += nbytes
    n = len(dev_areas)
    areas, iou, masks = host[:n], host[n].float().numpy(), host[n + 1:]
    T = len(target_shapes)
    return ([[masks[t * B + b].bool() for b in range(B)] for t in range(T)], [[areas[t * B + b].long() for b in range(B)] for t in range(T)], iou)


def sam(sam_model_dict, image, input_points=None, input_boxes=None, target_mask_shape=None, return_numpy=True, image_embeddings=None):
    """Reference ``models/sam.py:26-56`` with the image encoder replaced: ``sam_model_dict['sam_encoder']`` (``SamVisionEncoder`` above) makes the image
    embeddings unless ``image_embeddings`` brings them; ``sam_model`` (the caller's ``transformers.SamModel``) runs its prompt encoder and mask decoder
    on them.  The encoder's own dtype replaces the reference's ``torch.autocast`` for the encoder part.  target_mask_shape: (h, w).
    With ``sam_model`` a ``theatergen_amd.sam_decoder.SamModel`` the whole step stays on the device (``_sam_device``): the same return structure, the masks
    thresholded and resized by ``ops.sam_mask_post``."""
    import torch.nn.functional as F
    sam_model, proc = sam_model_dict["sam_model"], sam_model_dict["sam_processor"]
    if _on_device_route(sam_model):
        masks, _, iou = _sam_device(sam_model_dict, image, input_points, input_boxes, [tuple(target_mask_shape)], image_embeddings)
        return [m.numpy() if return_numpy else m for m in masks[0]], iou[0, 0]
    input_boxes = _listify_boxes(input_boxes)
    with torch.no_grad():
        inputs = proc(image, input_points=input_points, input_boxes=input_boxes, return_tensors="pt")
        if image_embeddings is None:
            enc = sam_model_dict["sam_encoder"]
            image_embeddings = enc(inputs["pixel_values"].to(enc.device))
        p0 = next(iter(sam_model.parameters()), None) if hasattr(sam_model, "parameters") else None
        dev, mdt = (p0.device, p0.dtype) if p0 is not None else (image_embeddings.device, image_embeddings.dtype)
        kw = {k: inputs[k].to(dev) for k in ("input_points", "input_boxes", "input_labels") if k in inputs and inputs[k] is not None}
        kw = {k: (v.to(mdt) if torch.is_floating_point(v) else v) for k, v in kw.items()}
        outputs = sam_model(image_embeddings=image_embeddings.to(device=dev, dtype=mdt), **kw)
        masks = proc.image_processor.post_process_masks(outputs.pred_masks.cpu().float(), inputs["original_sizes"].cpu(),
                                                        inputs["reshaped_input_sizes"].cpu())
        conf_scores = outputs.iou_scores.cpu().float().numpy()[0, 0]
    masks = [F.interpolate(m.type(torch.float), target_mask_shape, mode="bilinear").type(torch.bool) for m in masks]
    if return_numpy:
        masks = [m.numpy() for m in masks]
    return masks, conf_scores


def sam_point_input(sam_model_dict, image, input_points, **kwargs):
    return sam(sam_model_dict, image, input_points=input_points, **kwargs)


def sam_box_input(sam_model_dict, image, input_boxes, **kwargs):
    return sam(sam_model_dict, image, input_boxes=input_boxes, **kwargs)


def select_mask(masks, conf_scores, coarse_ious=None, rule="largest_over_conf", discourage_mask_below_confidence=0.85,
                discourage_mask_below_coarse_iou=0.2, verbose=False):
    """Reference ``models/sam.py:68-112`` on numpy arrays (masks: bool [n, h, w]), without its plotting: the largest mask wins, a mask whose
    confidence or coarse IoU is below its threshold is set back by the size of the largest one.  -> (mask, its confidence)."""
    masks = np.asarray(masks)
    conf_scores = np.asarray(conf_scores)
    mask_id = _select_mask_id(masks.sum(axis=(1, 2)), conf_scores, coarse_ious, rule, discourage_mask_below_confidence,
                              discourage_mask_below_coarse_iou, verbose)
    return masks[mask_id], conf_scores[mask_id]


def _select_mask_id(mask_sizes, conf_scores, coarse_ious, rule, discourage_mask_below_confidence, discourage_mask_below_coarse_iou, verbose):
    """``select_mask``'s rule on the mask sizes alone (the device route brings them from ``ops.sam_mask_post``)"""
    if rule != "largest_over_conf":
        raise ValueError(f"Unknown rule: {rule}")
    max_mask_size = np.max(mask_sizes)
    scores = mask_sizes - (conf_scores < discourage_mask_below_confidence) * max_mask_size
    if coarse_ious is not None:
        scores = scores - (np.asarray(coarse_ious) < discourage_mask_below_coarse_iou) * max_mask_size
    mask_id = int(np.argmax(scores))
    if verbose:
        print(f"mask_sizes: {mask_sizes}, scores: {scores}")
        print(f"Selected a mask with confidence: {conf_scores[mask_id]}, coarse_iou: {coarse_ious[mask_id] if coarse_ious is not None else None}")
    return mask_id


def sam_refine_characters(images, input_boxes, model_dict, height, width, discourage_mask_below_confidence, discourage_mask_below_coarse_iou,
                          verbose=False):
    """``sam_refine_attn`` (box prompts) for a list of characters at once — the companion of ``generate_characters``: one processor call, one encoder run and
    one decoder run at batch n, two ``ops.sam_mask_post`` launches per character, one copy back.  ``images[i]`` / ``input_boxes[i]``: what ``sam_refine_attn``
    takes as ``sam_input_image`` / ``input_boxes_w`` for character i (every character with the same number of boxes).  Needs the device route
    (``model_dict['sam_model']`` a ``theatergen_amd.sam_decoder.SamModel``).  -> four lists (mask, conf, mask_512, conf_512), entry i = ``sam_refine_attn`` of i."""
    if not _on_device_route(model_dict["sam_model"]):
        raise NotImplementedError("sam_refine_characters needs model_dict['sam_model'] to be a theatergen_amd.sam_decoder.SamModel (the device route)")
    images = list(images)
    boxes = np.concatenate([_prompt_array(b, 4, "input_boxes") for b in input_boxes], 0)
    if boxes.shape[0] != len(images):
        raise ValueError(f"sam_refine_characters: {len(images)} images, boxes for {boxes.shape[0]}")
    shapes = [(int(height / 8), int(width / 8)), (int(height), int(width))]
    masks, areas, iou = _sam_device(model_dict, images, None, boxes, shapes)
    out = ([], [], [], [])
    for b in range(len(images)):
        conf = iou[b, 0]
        for t in range(2):
            mid = _select_mask_id(areas[t][b][0].numpy(), conf, None, "largest_over_conf", discourage_mask_below_confidence,
                                  discourage_mask_below_coarse_iou, bool(verbose))
            out[2 * t].append(masks[t][b][0, mid].numpy())
            out[2 * t + 1].append(conf[mid])
    return out


def sam_refine_attn(input_boxes_w, obj_id, sam_input_image, token_attn_np, model_dict, height, width, H, W, use_box_input, gaussian_sigma,
                    mask_th_for_box, n_erode_dilate_mask_for_box, mask_th_for_point, discourage_mask_below_confidence,
                    discourage_mask_below_coarse_iou, verbose):
    """Reference ``models/sam.py:126-174``: the character's mask at latent resolution (height / 8, width / 8) and at image resolution.  The reference
    runs the whole SamModel once per target shape; here the image embeddings are computed ONCE and both shapes are served from them."""
    if use_box_input:
        raise NotImplementedError("sam_refine_attn: use_box_input=True cannot run in the reference either (its token_attn_np_smooth is the int 1, "
                                  "models/sam.py:134-141); only the box-prompt path (use_box_input=False) is supported")
    if _on_device_route(model_dict["sam_model"]):
        # one processor call, one encoder run, one decoder run, two post-processing launches, one host synchronisation
        r = sam_refine_characters([sam_input_image], [input_boxes_w], model_dict, height, width, discourage_mask_below_confidence,
                                  discourage_mask_below_coarse_iou, verbose)
        return r[0][0], r[1][0], r[2][0], r[3][0]
    H, W = int(height / 8), int(width / 8)
    emb = sam_image_embeddings(model_dict, sam_input_image)
    masks, conf_scores = sam_box_input(model_dict, image=sam_input_image, input_boxes=input_boxes_w, target_mask_shape=(H, W), image_embeddings=emb)
    masks_512, conf_scores1 = sam_box_input(model_dict, image=sam_input_image, input_boxes=input_boxes_w, target_mask_shape=(height, width),
                                            image_embeddings=emb)
    kw = dict(rule="largest_over_conf", discourage_mask_below_confidence=discourage_mask_below_confidence,
              discourage_mask_below_coarse_iou=discourage_mask_below_coarse_iou, verbose=bool(verbose))
    mask_selected, conf_score_selected = select_mask(masks[0][0], conf_scores, **kw)
    mask_selected_512, conf_score_selected_512 = select_mask(masks_512[0][0], conf_scores1, **kw)
    return mask_selected, conf_score_selected, mask_selected_512, conf_score_selected_512
