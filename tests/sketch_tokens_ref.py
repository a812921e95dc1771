"""fp64 restatement of the SVANet head with ``--sketch_attn tokens``: every video token attends to the sketch's tokens (the reference's
commented "V2 (7x7)" lines, cross_modal_transformer.py:129-135) in place of the one-token gate.  Composed from the oracle's pieces by
import (mha, layer_norm, position_embedding_sine, input_proj, query_self, query_cross); only the V2 half is written here, and
tests/test_sketch_tokens_ref.py pins it to torch.nn.MultiheadAttention running the commented lines literally.  Plain torch on the CPU.

Where this differs from the commented lines: they pass no key_padding_mask, this passes the padded sketch tokens (with an all-valid
mask the two are the same); a padded token's features are replaced by zeros before the projection, as the product does, so that
whatever they hold reaches nothing; positions are added to the keys only with ``args.use_sketch_pos``.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from oracle import svol_oracle as O
from svol_amd import synthetic as syn

# the device test's model: --backbone features --sketch_attn tokens, hidden_dim 64 / nheads 2 (d_h = 32), 2 layers, 8 queries,
# T = 4 frames of P = 6 tokens, input widths 48, Ls = 5 sketch tokens of which the last two of batch row 1 are padding
B, T, P, LS, PAD_ROW, PAD_TOKENS = 2, 4, 6, 5, 1, 2


def case_args(**over):
    a = dict(hidden_dim=64, nheads=2, num_layers=2, num_queries=8, num_queries_per_frame=2, num_frames=T, input_vid_dim=48,
             input_skch_dim=48, input_dropout=0.0, backbone='features', sketch_attn='tokens')
    a.update(over)
    return syn.head_args(**a)


def case_inputs(args, seed=1):
    """the model's inputs: src_sketch [B, Ls, 48], src_video [B, T, P, 48], src_sketch_mask [B, Ls] (already per token: one column per
    sketch token is what the mask expansion leaves alone), src_video_mask [B, T]"""
    r = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))   # noqa: E731
    smask = torch.ones((B, LS))
    smask[PAD_ROW, LS - PAD_TOKENS:] = 0.0
    return dict(src_sketch=f(B, LS, args.input_skch_dim), src_video=f(B, T, P, args.input_vid_dim), src_sketch_mask=smask,
                src_video_mask=torch.ones((B, T)))


def video_half_tokens(sd, p, h, src_vid, src_skch, vid_pos, skch_pos, skch_pad_mask):
    """the video half with the V2 lines: mem = norm1(MHA(src_vid + vid_pos, src_skch + skch_pos, src_skch) + src_vid), then :137-143"""
    o, _ = O.mha(src_vid + vid_pos, src_skch + skch_pos, src_skch, *O._mha_p(sd, p + 'sketch_video_cross_attn'), h,
                 key_padding_mask=skch_pad_mask)
    mem = O._ln(o + src_vid, sd, p + 'norm1')
    qk = mem + vid_pos
    o, _ = O.mha(qk, qk, mem, *O._mha_p(sd, p + 'content_self_attn'), h)
    mem = O._ln(o + mem, sd, p + 'norm2')
    return O._ln(mem + O.mlp_block(mem, sd, p + 'mlp1'), sd, p + 'norm3')


def forward(sd, args, src_sketch, src_sketch_mask, src_video, src_video_mask):
    """SVANet.forward in tokens mode at the HEAD's boundary (masks per token) -> the oracle's output dict.  Arithmetic in sd's dtype."""
    d, h, nl = args.hidden_dim, args.nheads, args.num_layers
    dtype = src_video.dtype
    vid = O.input_proj(src_video, sd, 'input_video_proj', args.n_input_proj)
    mask_video, mask_sketch = src_video_mask.bool(), src_sketch_mask.bool()
    pos_video = O.position_embedding_sine(mask_video, d, dtype)
    skch = O.input_proj(src_sketch.masked_fill(~mask_sketch[..., None], 0.0), sd, 'input_sketch_proj', args.n_input_proj)
    pos_sketch = O.position_embedding_sine(mask_sketch, d, dtype) if args.use_sketch_pos else torch.zeros_like(skch)
    Bn = vid.shape[0]
    query_pos = sd['query_embed.weight'].unsqueeze(0).expand(Bn, -1, -1)
    out = torch.zeros_like(query_pos)
    mem, hs = vid, []
    for i in range(nl):
        p = f'transformer.layers.{i}.'
        mem = video_half_tokens(sd, p, h, mem, skch, pos_video, pos_sketch, ~mask_sketch)
        out = O.query_cross(sd, p, h, O.query_self(sd, p, h, out, query_pos), mem, ~mask_video, pos_video, query_pos)
        hs.append(out)
    hs = torch.stack(hs)
    logits = O.linear(hs, sd['class_embed.weight'], sd['class_embed.bias'])
    x = hs
    for j in range(3):
        x = O.linear(x, sd[f'bbox_embed.layers.{j}.weight'], sd[f'bbox_embed.layers.{j}.bias'])
        if j < 2:
            x = torch.relu(x)
    boxes = torch.sigmoid(x)
    res = {'pred_logits': logits[-1], 'pred_boxes': boxes[-1]}
    if args.aux_loss:
        res['aux_outputs'] = [{'pred_logits': a, 'pred_boxes': b} for a, b in zip(logits[:-1], boxes[:-1])]
    return res


def model_forward(sd, args, inp):
    """the whole model with --backbone features: flatten the frames, expand the masks (n sketches: Ls // columns), then `forward`"""
    sk, vd = inp['src_sketch'], inp['src_video'].flatten(1, 2)
    smask = inp['src_sketch_mask'].repeat_interleave(sk.shape[1] // inp['src_sketch_mask'].shape[1], dim=1)
    vmask = inp['src_video_mask'].repeat_interleave(vd.shape[1] // inp['src_video'].shape[1], dim=1)
    dt = next(iter(sd.values())).dtype
    return forward(sd, args, sk.to(dt), smask, vd.to(dt), vmask)


def reference_run(args, inp, targets, indices=None, seed=1):
    """fp64 forward, criterion and backward on synth weights -> (outputs, loss dict, total, {head key: gradient or None}, indices)"""
    sd = {k: v.double().requires_grad_(True) for k, v in syn.synth_state_dict(args, seed=seed).items()}
    out = model_forward(sd, args, inp)
    ns = SimpleNamespace(**vars(args))
    if indices is None:
        ld, indices = O.set_criterion(ns, out, targets, return_indices=True)
    else:
        ld = O.set_criterion(ns, out, targets, indices=indices)
    tot = O.total_loss(args, ld)
    tot.backward()
    return out, ld, tot, {k: v.grad for k, v in sd.items()}, indices
