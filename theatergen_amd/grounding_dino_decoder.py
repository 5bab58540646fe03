"""GroundingDINO's two-stage query selection, decoder and box / class heads on the native kernels (``transformers``' ``GroundingDinoModel.forward`` after
the encoder, ``GroundingDinoDecoder`` and the last level of ``GroundingDinoForObjectDetection``'s heads; reference ``utils/detector.py``: the ``detect``
step of the character loop).

Token-major, storage dtype (bf16 / fp16) for the hidden states; the reference BOXES stay fp32 from the proposals to ``pred_boxes``: they go through one
logit / sigmoid round per layer and into a 2 pi / 10000^(..) phase, and ``ops.dino_box_update`` does the last layer of every box MLP, the logit, the
sigmoid, the per-level scaling and the sinusoidal embedding in one fp32 launch.

QUERY SELECTION (``two_stage``): the memory rows of padded tokens and of tokens whose proposal lies outside (0.01, 0.99) are zeroed (one
``masked_fill``), ``enc_output`` + ``enc_output_norm``, then ``ops.dino_contrastive`` gives the ROW MAXIMUM of the contrastive logits against the text states —
the [B, Nv, max_text_len] fp32 tensor ``transformers`` takes it from is never written — ``torch.topk`` on that fp32 vector picks ``num_queries`` tokens, and
``encoder_output_bbox_embed`` runs on the gathered rows only.  The proposal logits depend on the shapes and the padding mask alone: fp32 torch on the
device, ``inf`` where ``transformers`` puts it, cached per mask tensor.

DECODER LAYER, following ``transformers`` 5.x: self-attention with q | k from x + query_pos and v from x (q | k = x W^T + query_pos W^T, the second product
added through the GEMM's residual, as the encoder's text enhancer does; V^T with its pitch padded to a multiple of 8), text cross-attention with a finite
additive key mask, deformable cross-attention over the encoder memory (``ops.msdeform_attn`` with ``ref_dim`` 4 and the padding mask), fc1 + ReLU + fc2;
every one followed by ``ops.layernorm_add``.  The memory's value projections and the text K | V^T of ALL layers do not depend on the queries: one GEMM each
per forward.  ``query_pos`` is ``reference_points_head`` on the sinusoidal embedding ``ops.dino_box_update`` wrote; between layers ``bbox_embed[i]`` runs on
the un-normed state and feeds the next box update.

Nothing in ``forward`` synchronises with the host.  Parameter names are those of ``transformers.GroundingDinoForObjectDetection``.  Inference only.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops as _ops

_BIG = 1e30          # additive key mask of the text cross-attention: finite, an all-masked row is uniform, not NaN
_LAYER = ["self_attn.query", "self_attn.key", "self_attn.value", "self_attn.out_proj", "self_attn_layer_norm",
          "encoder_attn_text.query", "encoder_attn_text.key", "encoder_attn_text.value", "encoder_attn_text.out_proj", "encoder_attn_text_layer_norm",
          "encoder_attn.sampling_offsets", "encoder_attn.attention_weights", "encoder_attn.value_proj", "encoder_attn.output_proj",
          "encoder_attn_layer_norm", "fc1", "fc2", "final_layer_norm"]


def expected_names(config):
    """The parameter names ``from_state_dict`` takes, as ``GroundingDinoForObjectDetection.state_dict()`` spells them (its second spelling of the box
    heads, ``model.decoder.bbox_embed.*``, is the same tensors and is not taken)."""
    wb = lambda stem: [stem + ".weight", stem + ".bias"]                                             # noqa: E731
    names = []
    for i in range(int(config.decoder_layers)):
        for lin in _LAYER:
            names += wb(f"model.decoder.layers.{i}.{lin}")
        for j in range(3):
            names += wb(f"bbox_embed.{i}.layers.{j}")
    names += wb("model.decoder.layer_norm") + wb("model.enc_output") + wb("model.enc_output_norm")
    for j in range(2):
        names += wb(f"model.decoder.reference_points_head.layers.{j}")
    for j in range(3):
        names += wb(f"model.encoder_output_bbox_embed.layers.{j}")
    if getattr(config, "embedding_init_target", True):
        names.append("model.query_position_embeddings.weight")
    return set(names)


def check_config(config):
    """NotImplementedError naming the field for a config outside the kernels' envelope"""
    d, heads = int(config.d_model), int(config.decoder_attention_heads)
    bad = []
    if heads < 1 or d % heads or d // heads != 32:
        bad.append(f"d_model / decoder_attention_heads = {d} / {heads} (decoder head dim 32)")
    if d not in (128, 256):
        bad.append(f"d_model {d} (128 or 256: the box and contrastive kernels)")
    if int(config.decoder_n_points) != 4:
        bad.append(f"decoder_n_points {config.decoder_n_points} (4)")
    if not 1 <= int(config.num_feature_levels) <= 4:
        bad.append(f"num_feature_levels {config.num_feature_levels} (1 .. 4)")
    if getattr(config, "activation_function", "relu") != "relu":
        bad.append(f"activation_function {config.activation_function} (relu)")
    if not getattr(config, "two_stage", True):
        bad.append("two_stage False (True)")
    if int(getattr(config, "query_dim", 4)) != 4:
        bad.append(f"query_dim {config.query_dim} (4)")
    if getattr(config, "two_stage_bbox_embed_share", False):
        bad.append("two_stage_bbox_embed_share True (False)")
    if not 1 <= int(config.max_text_len) <= 256:
        bad.append(f"max_text_len {config.max_text_len} (1 .. 256)")
    if int(config.num_queries) < 1 or int(config.decoder_layers) < 1:
        bad.append(f"num_queries {config.num_queries} / decoder_layers {config.decoder_layers} (at least 1)")
    if bad:
        raise NotImplementedError("GroundingDinoDecoderHead: " + "; ".join(bad) + " has no kernel")


class _CountedOps:
    """``theatergen_amd.ops`` with every call tallied in ``owner.op_calls``: the count sits where the call is made"""

    def __init__(self, owner):
        self._owner = owner

    def __getattr__(self, name):
        fn = getattr(_ops, name)                      # looked up per call: a wrapper put on the module (the timing script's) is honoured

        def call(*args, **kwargs):
            self._owner.op_calls += 1
            return fn(*args, **kwargs)
        return call


def _pad8(n):
    return (int(n) + 7) // 8 * 8


class GroundingDinoDecoderHead:
    """``forward(vision_memory, vision_valid_mask, text_states, text_token_mask, spatial_shapes_list, valid_ratios)`` -> ``logits`` fp32
    [B, Q, max_text_len], ``pred_boxes`` fp32 [B, Q, 4], ``topk_proposals`` int64 [B, Q] and the per-layer states."""

    def __init__(self, config, params, device="cuda", dtype=torch.bfloat16):
        check_config(config)
        want = expected_names(config)
        missing, unexpected = sorted(want - set(params)), sorted(set(params) - want)
        if missing or unexpected:
            raise RuntimeError(f"state dict mismatch: missing {missing[:5]}... unexpected {unexpected[:5]}...")
        if dtype not in (torch.bfloat16, torch.float16):
            raise RuntimeError(f"GroundingDinoDecoderHead: storage dtype {dtype} unsupported (bf16 / fp16)")
        self.config = config
        self.device, self.dtype = torch.device(device), dtype
        self.d, self.heads, self.levels = int(config.d_model), int(config.decoder_attention_heads), int(config.num_feature_levels)
        self.n_layers, self.Q, self.max_text_len = int(config.decoder_layers), int(config.num_queries), int(config.max_text_len)
        self.eps = float(getattr(config, "layer_norm_eps", 1e-5))
        self.init_target = bool(getattr(config, "embedding_init_target", True))
        f32 = {k: v.detach().to(device=self.device, dtype=torch.float32) for k, v in params.items()}
        st = lambda t: t.to(dtype).contiguous()                                                       # noqa: E731
        wb = lambda name: (st(f32[name + ".weight"]), st(f32[name + ".bias"]))                       # noqa: E731
        cat = lambda names, s: st(torch.cat([f32[n + s] for n in names], 0))                         # noqa: E731

        def box_mlp(stem):
            """(layer 0, layer 1, w3 storage dtype [4, d], b3 fp32 [4] = the stored bias, which the kernel adds in fp32)"""
            return wb(stem + ".layers.0"), wb(stem + ".layers.1"), st(f32[stem + ".layers.2.weight"]), \
                st(f32[stem + ".layers.2.bias"]).float().contiguous()
        self.layers = []
        for i in range(self.n_layers):
            p = f"model.decoder.layers.{i}."
            sa, ta, da = p + "self_attn.", p + "encoder_attn_text.", p + "encoder_attn."
            self.layers.append(dict(
                sa_wqkv=cat([sa + "query", sa + "key", sa + "value"], ".weight"), sa_bqkv=cat([sa + "query", sa + "key", sa + "value"], ".bias"),
                sa_wqk=cat([sa + "query", sa + "key"], ".weight"), sa_o=wb(sa + "out_proj"), sa_ln=wb(p + "self_attn_layer_norm"),
                ta_q=wb(ta + "query"), ta_o=wb(ta + "out_proj"), ta_ln=wb(p + "encoder_attn_text_layer_norm"),
                da_wol=cat([da + "sampling_offsets", da + "attention_weights"], ".weight"),
                da_bol=cat([da + "sampling_offsets", da + "attention_weights"], ".bias"),
                da_o=wb(da + "output_proj"), da_ln=wb(p + "encoder_attn_layer_norm"),
                fc1=wb(p + "fc1"), fc2=wb(p + "fc2"), ln=wb(p + "final_layer_norm"), box=box_mlp(f"bbox_embed.{i}")))
        lay = [f"model.decoder.layers.{i}." for i in range(self.n_layers)]
        # query-independent projections of all layers, one GEMM each per forward: the memory's values; the text K of every layer | the text V of every layer
        self.w_val = cat([p + "encoder_attn.value_proj" for p in lay], ".weight")
        self.b_val = cat([p + "encoder_attn.value_proj" for p in lay], ".bias")
        tkv = [p + "encoder_attn_text.key" for p in lay] + [p + "encoder_attn_text.value" for p in lay]
        self.w_tkv, self.b_tkv = cat(tkv, ".weight"), cat(tkv, ".bias")
        self.dec_ln = wb("model.decoder.layer_norm")
        self.rph = (wb("model.decoder.reference_points_head.layers.0"), wb("model.decoder.reference_points_head.layers.1"))
        self.enc_output, self.enc_output_norm = wb("model.enc_output"), wb("model.enc_output_norm")
        self.enc_box = box_mlp("model.encoder_output_bbox_embed")
        self.query_embed = st(f32["model.query_position_embeddings.weight"]) if self.init_target else None
        self._prop_cache = {}
        self._buffers = {}
        self._targets = {}
        self.op_calls = 0              # calls into the native library so far (a tally kept here, not a count of kernel launches)
        self.ops = _CountedOps(self)
        self.taps = None               # a list: receives ("select", topk, ref) and ("layer", i, normed state, ref) (the tests' per-stage checks)

    @classmethod
    def from_state_dict(cls, config, state_dict, device="cuda", dtype=torch.bfloat16):
        """``state_dict``: of a ``GroundingDinoForObjectDetection`` (filtered to the entries this part takes; tied or untied box heads are read as they are
        held), or of a ``GroundingDinoModel`` whose decoder carries the box heads (``decoder.bbox_embed.*``).  A missing or unexpected name is a RuntimeError."""
        if not any(k.startswith("model.") for k in state_dict):
            state_dict = {("bbox_embed." + k[len("decoder.bbox_embed."):] if k.startswith("decoder.bbox_embed.") else "model." + k): v
                          for k, v in state_dict.items()}
        take = ("model.decoder.", "model.enc_output.", "model.enc_output_norm.", "model.encoder_output_bbox_embed.", "model.query_position_embeddings.",
                "bbox_embed.")
        sub = {k: v for k, v in state_dict.items() if k.startswith(take) and not k.startswith("model.decoder.bbox_embed.")}
        return cls(config, sub, device, dtype)

    # ---- per-forward constants ---------------------------------------------------------------------------------------------------------------
    def proposals(self, shapes, valid):
        """``GroundingDinoModel.generate_encoder_output_proposals`` without the features -> (proposal logits fp32 [B * Nv, 4], ``inf`` for a padded token
        or a proposal outside (0.01, 0.99); bool [B * Nv, 1], True = such a token, whose memory row is zeroed).  ``valid`` bool
        [B, Nv], True = a real token.  Cached per mask TENSOR (same object, same ``_version``), as the encoder caches its reference points."""
        key = (id(valid), valid._version, tuple(shapes))
        hit = self._prop_cache.get(key)
        if hit is None or hit[0] is not valid:
            if len(self._prop_cache) >= 8:
                self._prop_cache.clear()
            dev = self.device
            v = valid.to(dev).bool()
            B = v.shape[0]
            props, pos = [], 0
            for level, (h, w) in enumerate(shapes):
                m = v[:, pos:pos + h * w].view(B, h, w)
                vh, vw = m[:, :, 0].sum(1), m[:, 0, :].sum(1)
                gy, gx = torch.meshgrid(torch.linspace(0, h - 1, h, dtype=torch.float32, device=dev),
                                        torch.linspace(0, w - 1, w, dtype=torch.float32, device=dev), indexing="ij")
                grid = torch.stack((gx, gy), -1)
                scale = torch.stack((vw, vh), 1).view(B, 1, 1, 2)
                grid = (grid[None].expand(B, -1, -1, -1) + 0.5) / scale
                wh = torch.ones_like(grid) * 0.05 * (2.0 ** level)
                props.append(torch.cat((grid, wh), -1).view(B, -1, 4))
                pos += h * w
            p = torch.cat(props, 1)
            ok = ((p > 0.01) & (p < 0.99)).all(-1, keepdim=True) & v[..., None]
            logit = torch.log(p / (1 - p)).masked_fill(~ok, float("inf"))
            hit = (valid, logit.reshape(-1, 4).contiguous(), (~ok).reshape(-1, 1).contiguous())
            self._prop_cache[key] = hit
        return hit[1], hit[2]

    def _zeros(self, name, shape):
        """a persistent zero-initialised buffer per (name, shape): the kernels that write it never touch its padding, which stays zero"""
        key = (name,) + tuple(shape)
        buf = self._buffers.get(key)
        if buf is None:
            if len(self._buffers) >= 32:
                self._buffers.clear()
            buf = torch.zeros(shape, dtype=self.dtype, device=self.device)
            self._buffers[key] = buf
        return buf

    def _target(self, B):
        t = self._targets.get(B)
        if t is None:
            t = self._targets[B] = self.query_embed[None].expand(B, -1, -1).reshape(B * self.Q, self.d).contiguous()
        return t

    def _mlp2(self, x, box):
        """the first two layers of a box MLP, each with its ReLU"""
        (w0, b0), (w1, b1) = box[0], box[1]
        return self.ops.relu(self.ops.linear(self.ops.relu(self.ops.linear(x, w0, b0)), w1, b1))

    # ---- query selection -------------------------------------------------------------------------------------------------------------------------
    def select(self, mem, valid, text, token_mask, shapes, valid_ratios, B, Nv, topk=None):
        """-> (topk int64 [B, Q], gathered object queries [B * Q, d], ref fp32 [B * Q, 4], ref_levels fp32 [B * Q, L, 4], pos_in [B * Q, 2 d]).
        ``topk``: the selected proposals in rank order, given by the caller instead of taken from the scores."""
        logit, drop = self.proposals(shapes, valid)
        oq = self.ops.linear(mem.masked_fill(drop, 0), self.enc_output[0], self.enc_output[1])
        oq = self.ops.layernorm(oq, self.enc_output_norm[0], self.enc_output_norm[1], self.eps)
        if topk is None:
            _, score = self.ops.dino_contrastive(oq.view(B, Nv, self.d), text, token_mask, self.max_text_len, logits=False, row_max=True)
            topk = torch.topk(score, self.Q, dim=1)[1]
        elif tuple(topk.shape) != (B, self.Q) or topk.dtype != torch.int64 or topk.device.type != self.device.type:
            raise ValueError(f"GroundingDinoDecoderHead: topk_proposals must be an int64 tensor [{B}, {self.Q}] on {self.device}")
        flat = (topk + torch.arange(B, device=self.device)[:, None] * Nv).reshape(-1)
        g = oq.index_select(0, flat)
        ref, ref_levels, pos_in = self.ops.dino_box_update(self._mlp2(g, self.enc_box), self.enc_box[2], self.enc_box[3], logit.index_select(0, flat), False,
                                                      self.Q, valid_ratios, ref_levels=True, pos_in=True)
        return topk, g, ref, ref_levels, pos_in

    # ---- the decoder ---------------------------------------------------------------------------------------------------------------------------------
    def memory_context(self, mem, valid, text, token_mask, shapes, B, Nv, Lt):
        """what the layers share: the value projections of all layers [B * Nv, layers * d], the text K [B * Lt (+ spare), layers * d] and V^T
        [B, layers * d, pad8(Lt)] of all layers, the padding mask of the memory (uint8, 1 = padding) and the additive text key mask"""
        d, nl = self.d, self.n_layers
        Ltp = _pad8(Lt)
        vals = self.ops.linear(mem, self.w_val, self.b_val)
        tk = self._zeros("tk", (B * Lt + 64, nl * d))             # spare rows behind the last item: a key tile may read past an item's rows
        tvt = self._zeros("tvt", (B, nl * d, Ltp))                # columns [Lt, pad8(Lt)) stay zero: 0 * V must not be NaN
        self.ops.gemm(text, self.w_tkv, B * Lt, 2 * nl * d, d, bias=self.b_tkv, rows_per_batch=Lt, out=tk[:B * Lt], n_split=nl * d, out_t=tvt, ldt=Ltp)
        add_mask = ((~token_mask).to(torch.float32) * -_BIG).reshape(B, 1, 1, Lt).contiguous()
        return SimpleNamespace(vals=vals, tk=tk, tvt=tvt, Ltp=Ltp, vmask=(~valid).to(torch.uint8).contiguous(), add_mask=add_mask, shapes=shapes, B=B,
                               Nv=Nv, Lt=Lt)

    def _layer(self, i, x, pos_in, ref_levels, c):
        ly, d, H, Q, B, nl = self.layers[i], self.d, self.heads, self.Q, c.B, self.n_layers
        M, Qp, scale = B * Q, _pad8(Q), 32 ** -0.5
        qpos = self.ops.linear(self.ops.relu(self.ops.linear(pos_in, self.rph[0][0], self.rph[0][1])), self.rph[1][0], self.rph[1][1])
        # self-attention
        qk0 = self._zeros("sa_qk0", (M + 64, 2 * d))
        qk = self._zeros("sa_qk", (M + 64, 2 * d))
        vt = self._zeros("sa_vt", (B, d, Qp))
        self.ops.gemm(x, ly["sa_wqkv"], M, 3 * d, d, bias=ly["sa_bqkv"], rows_per_batch=Q, out=qk0[:M], n_split=2 * d, out_t=vt, ldt=Qp)
        self.ops.linear(qpos, ly["sa_wqk"], None, res=qk0[:M], out=qk[:M])
        o = torch.empty((M, d), dtype=self.dtype, device=self.device)
        self.ops.attention(qk, 2 * d, Q * 2 * d, qk[:, d:], 2 * d, Q * 2 * d, vt, Qp, d * Qp, Q, B, H, 32, Q, scale, o, d, Q * d)
        x = self.ops.layernorm_add(self.ops.linear(o, ly["sa_o"][0], ly["sa_o"][1]), x, ly["sa_ln"][0], ly["sa_ln"][1], self.eps)
        # text cross-attention
        q = self.ops.linear(self.ops.add(x, qpos), ly["ta_q"][0], ly["ta_q"][1])
        o = torch.empty((M, d), dtype=self.dtype, device=self.device)
        self.ops.attention(q, d, Q * d, c.tk[:, i * d:], nl * d, c.Lt * nl * d, c.tvt[:, i * d:], c.Ltp, nl * d * c.Ltp, c.Lt, B, H, 32, Q,
                      scale, o, d, Q * d, mask=c.add_mask)
        x = self.ops.layernorm_add(self.ops.linear(o, ly["ta_o"][0], ly["ta_o"][1]), x, ly["ta_ln"][0], ly["ta_ln"][1], self.eps)
        # deformable cross-attention over the encoder memory
        n_off = H * self.levels * 8
        ol = self.ops.linear(self.ops.add(x, qpos), ly["da_wol"], ly["da_bol"])                                 # offsets | logits
        o = torch.empty((M, d), dtype=self.dtype, device=self.device)
        self.ops.msdeform_attn(c.vals[:, i * d:(i + 1) * d], nl * d, c.Nv * nl * d, c.shapes, ol, ol.stride(0), ol[:, n_off:], ol.stride(0),
                          ref_levels.view(B, Q, self.levels, 4), B, H, Q, o, d, Q * d, value_mask=c.vmask)
        x = self.ops.layernorm_add(self.ops.linear(o, ly["da_o"][0], ly["da_o"][1]), x, ly["da_ln"][0], ly["da_ln"][1], self.eps)
        # feed-forward
        y = self.ops.linear(self.ops.relu(self.ops.linear(x, ly["fc1"][0], ly["fc1"][1])), ly["fc2"][0], ly["fc2"][1])
        return self.ops.layernorm_add(y, x, ly["ln"][0], ly["ln"][1], self.eps)

    def decode(self, x, ref, ref_levels, pos_in, c, valid_ratios):
        """the decoder layers with the box refinement between them -> (un-normed last state [B * Q, d], [normed state per layer], [ref after each layer],
        the ref that ENTERED the last layer)"""
        normed, refs = [], []
        for i in range(self.n_layers):
            x = self._layer(i, x, pos_in, ref_levels, c)
            box = self.layers[i]["box"]
            last = i == self.n_layers - 1
            prior = ref
            ref, ref_levels, pos_in = self.ops.dino_box_update(self._mlp2(x, box), box[2], box[3], prior, True, self.Q, valid_ratios,
                                                          ref_levels=not last, pos_in=not last)
            normed.append(self.ops.layernorm(x, self.dec_ln[0], self.dec_ln[1], self.eps))
            refs.append(ref)
            if self.taps is not None:
                self.taps.append(("layer", i, normed[-1].view(c.B, self.Q, self.d), ref.view(c.B, self.Q, 4)))
        return x, normed, refs, prior

    def _check_inputs(self, vision_memory, text_states, shapes):
        if not vision_memory.is_cuda:
            raise RuntimeError("theatergen_amd GroundingDINO decoder runs on the GPU only (no CPU fallback)")
        if len(shapes) != self.levels:
            raise ValueError(f"GroundingDinoDecoderHead: {len(shapes)} levels given, the config has {self.levels}")
        B, Nv, d = vision_memory.shape
        if d != self.d or sum(h * w for h, w in shapes) != Nv or text_states.shape[0] != B or text_states.shape[2] != d:
            raise ValueError(f"GroundingDinoDecoderHead: memory {tuple(vision_memory.shape)} / text {tuple(text_states.shape)} do not match d_model "
                             f"{self.d} and the levels {shapes}")
        if not 1 <= text_states.shape[1] <= self.max_text_len:
            raise ValueError(f"GroundingDinoDecoderHead: {text_states.shape[1]} text tokens, max_text_len is {self.max_text_len}")
        if Nv < self.Q:
            raise ValueError(f"GroundingDinoDecoderHead: {Nv} memory tokens, num_queries is {self.Q}")

    # ---- forward -----------------------------------------------------------------------------------------------------------------------------------
    def forward(self, vision_memory, vision_valid_mask, text_states, text_token_mask, spatial_shapes_list, valid_ratios, output_attentions=None,
                topk_proposals=None):
        """``vision_memory`` [B, Nv, d] and ``text_states`` [B, Lt, d]: the encoder's two outputs; ``vision_valid_mask`` bool [B, Nv], True = a real token
        (``transformers``' ``mask_flatten``; None = all); ``text_token_mask`` bool [B, Lt], True = a real token; ``valid_ratios`` fp32 [B, L, 2].
        ``topk_proposals`` int64 [B, Q]: take these proposals, in this rank order, instead of the top scores.  With ``embedding_init_target`` the content
        query of a proposal is ``query_position_embeddings[rank]``, and scores a rounding apart may swap ranks: a caller who needs the order of another
        run (the tests, against the fp32 golden) passes it."""
        if output_attentions:
            raise NotImplementedError("GroundingDinoDecoderHead: output_attentions=True (no attention matrix exists in memory)")
        shapes = [(int(h), int(w)) for h, w in spatial_shapes_list]
        self._check_inputs(vision_memory, text_states, shapes)
        B, Nv, d = vision_memory.shape
        Lt, Q = int(text_states.shape[1]), self.Q
        with torch.no_grad():
            dev, dt = self.device, self.dtype
            mem = vision_memory.to(device=dev, dtype=dt).reshape(B * Nv, d).contiguous()
            text = text_states.to(device=dev, dtype=dt).contiguous()
            valid = vision_valid_mask if vision_valid_mask is not None else torch.ones((B, Nv), dtype=torch.bool, device=dev)
            if valid.device != dev or valid.dtype != torch.bool:
                valid = valid.to(dev).bool()
            token_mask = text_token_mask.to(dev).bool() if text_token_mask is not None else torch.ones((B, Lt), dtype=torch.bool, device=dev)
            vr = valid_ratios.to(device=dev, dtype=torch.float32).contiguous()
            topk, g, ref0, ref_levels, pos_in = self.select(mem, valid, text, token_mask, shapes, vr, B, Nv, topk_proposals)
            if self.taps is not None:
                self.taps.append(("select", topk, ref0.view(B, Q, 4)))
            c = self.memory_context(mem, valid, text.reshape(B * Lt, d), token_mask, shapes, B, Nv, Lt)
            x, normed, refs, prior = self.decode(self._target(B) if self.init_target else g, ref0, ref_levels, pos_in, c, vr)
            logits, _ = self.ops.dino_contrastive(normed[-1].view(B, Q, d), text, token_mask, self.max_text_len)
            box = self.layers[-1]["box"]
            boxes, _, _ = self.ops.dino_box_update(self._mlp2(normed[-1], box), box[2], box[3], prior, True, Q)
        return SimpleNamespace(logits=logits, pred_boxes=boxes.view(B, Q, 4), topk_proposals=topk, init_reference_points=ref0.view(B, Q, 4),
                               intermediate_hidden_states=torch.stack([n.view(B, Q, d) for n in normed], 1),
                               intermediate_reference_points=torch.stack([r.view(B, Q, 4) for r in refs], 1),
                               last_hidden_state=normed[-1].view(B, Q, d))

    __call__ = forward

    # ---- transformers integration --------------------------------------------------------------------------------------------------------------
    def attach(self, hf_model):
        """Make a ``transformers`` ``GroundingDinoModel`` / ``GroundingDinoForObjectDetection`` use this decoder: its ``decoder`` is replaced by a thin module
        that runs the layers and the box refinement here and returns a ``GroundingDinoDecoderOutput`` in the dtype of the model behind it; ``transformers``
        keeps its own query selection and heads.  Composes with ``GroundingDinoVisionFront.attach`` and ``GroundingDinoFusionEncoder.attach``."""
        core = hf_model.model if hasattr(hf_model, "model") and hasattr(hf_model.model, "decoder") else hf_model
        if not hasattr(core, "decoder") or not hasattr(core, "enc_output"):
            raise TypeError("attach: a two-stage transformers GroundingDinoModel or GroundingDinoForObjectDetection expected")
        p0 = next(iter(core.enc_output.parameters()), None)
        core.decoder = _DecoderModule(self, p0.dtype if p0 is not None else self.dtype)
        return hf_model


class _DecoderModule(nn.Module):
    def __init__(self, head, out_dtype):
        super().__init__()
        self._head, self.out_dtype = [head], out_dtype              # a list: the head is no nn.Module and is not to be registered

    def forward(self, inputs_embeds, vision_encoder_hidden_states, vision_encoder_attention_mask=None, text_encoder_hidden_states=None,
                text_encoder_attention_mask=None, reference_points=None, spatial_shapes=None, spatial_shapes_list=None, level_start_index=None,
                valid_ratios=None, self_attn_mask=None, output_attentions=None, output_hidden_states=None, return_dict=None, **kwargs):
        from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoDecoderOutput, encode_sinusoidal_position_embedding
        hd = self._head[0]
        if output_attentions:
            raise NotImplementedError("GroundingDinoDecoderHead: output_attentions=True (no attention matrix exists in memory)")
        if output_hidden_states:
            raise NotImplementedError("GroundingDinoDecoderHead: output_hidden_states=True through attach (the intermediate states are returned)")
        if self_attn_mask is not None:
            raise NotImplementedError("GroundingDinoDecoderHead: self_attn_mask")
        if reference_points is None or reference_points.shape[-1] != 4 or spatial_shapes_list is None or valid_ratios is None:
            raise ValueError("GroundingDinoDecoderHead: reference_points [B, Q, 4], spatial_shapes_list and valid_ratios are required")
        shapes = [(int(h), int(w)) for h, w in spatial_shapes_list]
        hd._check_inputs(vision_encoder_hidden_states, text_encoder_hidden_states, shapes)
        B, Nv, d = vision_encoder_hidden_states.shape
        Lt, Q = int(text_encoder_hidden_states.shape[1]), hd.Q
        if tuple(inputs_embeds.shape) != (B, Q, d):
            raise ValueError(f"GroundingDinoDecoderHead: inputs_embeds {tuple(inputs_embeds.shape)}, expected {(B, Q, d)}")
        with torch.no_grad():
            dev, dt = hd.device, hd.dtype
            mem = vision_encoder_hidden_states.to(device=dev, dtype=dt).reshape(B * Nv, d).contiguous()
            text = text_encoder_hidden_states.to(device=dev, dtype=dt).reshape(B * Lt, d).contiguous()
            valid = (vision_encoder_attention_mask.to(dev).bool() if vision_encoder_attention_mask is not None
                     else torch.ones((B, Nv), dtype=torch.bool, device=dev))
            token_mask = (~text_encoder_attention_mask.to(dev).bool() if text_encoder_attention_mask is not None
                          else torch.ones((B, Lt), dtype=torch.bool, device=dev))
            vr = valid_ratios.to(device=dev, dtype=torch.float32).contiguous()
            # the first layer's box operands from the caller's reference points, fp32 torch (GroundingDinoDecoder.forward's own three lines)
            ref = reference_points.to(device=dev, dtype=torch.float32).reshape(B * Q, 4).contiguous()
            ref_levels = (ref.view(B, Q, 1, 4) * torch.cat([vr, vr], -1)[:, None]).contiguous()
            pos_in = encode_sinusoidal_position_embedding(ref_levels[:, :, 0, :], num_pos_feats=d // 2).reshape(B * Q, 2 * d).to(dt).contiguous()
            c = hd.memory_context(mem, valid, text, token_mask, shapes, B, Nv, Lt)
            x = inputs_embeds.to(device=dev, dtype=dt).reshape(B * Q, d).contiguous()
            _, normed, refs, _ = hd.decode(x, ref, ref_levels.view(B * Q, hd.levels, 4), pos_in, c, vr)
            od = self.out_dtype
            inter = torch.stack([n.view(B, Q, d) for n in normed], 1).to(od)
            inter_ref = torch.stack([r.view(B, Q, 4) for r in refs], 1).to(od)
            last = inter[:, -1]
        if return_dict is not None and not return_dict:
            return (last, inter, inter_ref)
        return GroundingDinoDecoderOutput(last_hidden_state=last, intermediate_hidden_states=inter, intermediate_reference_points=inter_ref,
                                          hidden_states=None, attentions=None)
