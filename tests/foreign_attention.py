"""Test infrastructure: a diffusers-0.21.4-shaped ``Attention`` and a ``set_attn_processor`` host that are NOT theatergen_amd classes.

``ForeignAttention`` carries exactly the instance attributes the reference class assigns in its constructor
(/root/reference/ip_adapter/attention_processor.py:51-148): ``upcast_attention``, ``upcast_softmax``, ``rescale_output_factor``,
``residual_connection``, ``_from_deprecated_attn_block``, ``scale_qk``, ``scale``, ``heads``, ``sliceable_head_dim``,
``added_kv_proj_dim``, ``only_cross_attention``, ``group_norm``, ``spatial_norm``, ``norm_cross``, ``to_q``, ``to_k``, ``to_v``, ``to_out``,
``processor`` — and nothing else: no ``inner_dim`` (a constructor LOCAL in the reference, :52), no ``dim_head``, no packed-weight helpers.
Its compute helpers (``head_to_batch_dim``, ``get_attention_scores`` ...) are deliberately absent: a processor that needs them is not a
drop-in for a kernel-backed path.  ``ForeignUNet.set_attn_processor`` distributes a ``{name.processor: processor}`` dict the way
diffusers' ``UNet2DConditionModel.set_attn_processor`` does (reference models/unet_2d_condition.py:536-568), which is what
``IPAdapter.set_ip_adapter`` calls (ip_adapter/ip_adapter.py:95-119).
"""
import torch.nn as nn


class ForeignAttention(nn.Module):
    def __init__(self, query_dim, cross_attention_dim=None, heads=8, dim_head=64, dropout=0.0, bias=False, upcast_attention=False,
                 upcast_softmax=False, cross_attention_norm=None, cross_attention_norm_num_groups=32, norm_num_groups=None, out_bias=True,
                 scale_qk=True, eps=1e-5, rescale_output_factor=1.0, residual_connection=False, processor=None):
        super().__init__()
        inner = dim_head * heads                                  # a LOCAL, as in the reference
        cross = cross_attention_dim if cross_attention_dim is not None else query_dim
        self.upcast_attention = upcast_attention
        self.upcast_softmax = upcast_softmax
        self.rescale_output_factor = rescale_output_factor
        self.residual_connection = residual_connection
        self._from_deprecated_attn_block = False
        self.scale_qk = scale_qk
        self.scale = dim_head ** -0.5 if scale_qk else 1.0
        self.heads = heads
        self.sliceable_head_dim = heads
        self.added_kv_proj_dim = None
        self.only_cross_attention = False
        self.group_norm = nn.GroupNorm(num_channels=query_dim, num_groups=norm_num_groups, eps=eps, affine=True) if norm_num_groups else None
        self.spatial_norm = None
        if cross_attention_norm is None:
            self.norm_cross = None
        elif cross_attention_norm == "layer_norm":
            self.norm_cross = nn.LayerNorm(cross)
        else:
            self.norm_cross = nn.GroupNorm(num_channels=cross, num_groups=cross_attention_norm_num_groups, eps=1e-5, affine=True)
        self.to_q = nn.Linear(query_dim, inner, bias=bias)
        self.to_k = nn.Linear(cross, inner, bias=bias)
        self.to_v = nn.Linear(cross, inner, bias=bias)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim, bias=out_bias), nn.Dropout(dropout)])
        self.processor = processor

    def set_processor(self, processor):
        if hasattr(self, "processor") and isinstance(self.processor, nn.Module) and not isinstance(processor, nn.Module):
            self._modules.pop("processor")
        self.processor = processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **cross_attention_kwargs):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask,
                              **cross_attention_kwargs)


class _Block(nn.Module):
    def __init__(self, attn1, attn2):
        super().__init__()
        self.attn1, self.attn2 = attn1, attn2


class ForeignUNet(nn.Module):
    """two transformer blocks' worth of attention modules under diffusers-style names; only the processor plumbing is modelled"""

    def __init__(self, blocks):
        super().__init__()
        self.down_blocks = nn.ModuleList([nn.ModuleDict({"attentions": nn.ModuleList([nn.ModuleDict({"transformer_blocks": nn.ModuleList([b])})])})
                                          for b in blocks])

    @property
    def attn_processors(self):
        procs = {}

        def rec(name, module):
            if hasattr(module, "set_processor"):
                procs[f"{name}.processor"] = module.processor
            for sub, child in module.named_children():
                if sub != "processor":
                    rec(f"{name}.{sub}", child)

        for name, module in self.named_children():
            rec(name, module)
        return procs

    def set_attn_processor(self, processor):
        count = len(self.attn_processors.keys())
        if isinstance(processor, dict) and len(processor) != count:
            raise ValueError(f"A dict of processors was passed, but the number of processors {len(processor)} does not match the number "
                             f"of attention layers: {count}.")

        def rec(name, module, processor):
            if hasattr(module, "set_processor"):
                module.set_processor(processor if not isinstance(processor, dict) else processor.pop(f"{name}.processor"))
            for sub, child in module.named_children():
                if sub != "processor":
                    rec(f"{name}.{sub}", child, processor)

        for name, module in self.named_children():
            rec(name, module, processor)


class ReferenceShapedAttention(ForeignAttention):
    """``ForeignAttention`` with the forward of the reference's OWN ``Attention`` (ip_adapter/attention_processor.py:156-167), which also hands its
    processor ``return_attntion_probs`` (its spelling); the keywords it sends are checked against tests/golden/attention_attrs.npz"""

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, return_attntion_probs=False, **cross_attention_kwargs):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask,
                              return_attntion_probs=return_attntion_probs, **cross_attention_kwargs)
