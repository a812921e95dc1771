"""Model assembly (reference lib/modeling/model.py:8-44): backbone -> mask expansion -> head.

``build_model(args)`` / ``SketchLocalizationModel.forward(src_sketch, src_video, src_sketch_mask,
src_video_mask)`` keep the reference's signatures and the ``backbone.`` / ``head.`` state-dict
prefixes.  The online extractors also take RAW frames — uint8 ``[B,T,H,W,3]`` / ``[B,1,H,W,3]`` or lists of ``[T,H_b,W_b,3]`` — and
resize and normalise them on the device (svol_amd/ingest.py; ``args.pixel_preset`` overrides the backbone's preset; ``args.sketch_filter`` / ``args.sketch_invert`` give the sketch another of
Pillow's filters / inverted source bytes, and a raw sketch may be grey, ``[B,1,H,W]``).  ``--backbone features`` plugs pre-extracted features in at the measured boundary;
``--backbone vit`` runs the ViT-B/16 extractor of ``backbone.py`` on the device for every frame and the sketch
(SURVEY.md §8 f1), frozen unless ``args.train_backbone`` is 1 (``--finetune_layers K``: only the last K layers and the final
LayerNorm train, as preprocess/sketch_vit_finetune.py does).  ``--compute_dtype fp16`` gives both ViT extractors fp16 operands, in the
frozen and the trainable path alike; a bf16 or fp32 head keeps the bf16 extractors (the short-sequence attention kernels have no fp32
form).  Its default stays frozen, unlike the ResNet's: the reference's
ViT backbone cannot run as shipped (``device`` is undefined in ViTBackbone.forward, backbone.py:30), so no reference run
trains it, and existing users of ``--backbone vit`` keep the frozen extractors; ``--backbone resnet`` the ResNet-34 / ResNet-18 extractors of ``resnet.py`` (f4)
(``--backbone resnet50``: the reference's third pair, ResNet-50 for frames and sketch, 2048-wide features, same switches), frozen by default,
trained with the head when ``args.train_backbone`` is set (what the reference's train.py does); they run in ``args.compute_dtype``,
fp16 included in both modes.
"""
from __future__ import annotations

import torch
from torch import nn

from .svanet import build_svanet


class FeatureBackbone(nn.Module):
    """Identity feature 'backbone': src_sketch [B,Ls,Dskch], src_video [B,T,P,Dvid] (or [B,T*P,Dvid])
    are already features.  Returns (sketch [B,Ls,D], video [B,T*P,D]) like backbone.py:72-89."""

    def forward(self, src_sketch, src_video):
        if isinstance(src_video, (list, tuple)) or src_video.dtype == torch.uint8 or getattr(src_sketch, 'dtype', None) == torch.uint8:
            raise TypeError("--backbone features takes pre-extracted float features; raw uint8 frames need an online extractor "
                            "(--backbone resnet / vit), whose FrameIngest resizes and normalises them on the device")
        if src_video.dim() == 4:
            src_video = src_video.flatten(1, 2)
        return src_sketch, src_video


SKETCH_TOKENS = ('pooled', 'grid')


def _sketch_tokens(args):
    """``args.sketch_tokens`` (set on the args object like pixel_preset, no command-line flag): 'pooled' = one token per sketch, what the
    reference's extractors hand over; 'grid' = every token of the sketch extractor, 7 x 7 = 49 of a ResNet (no average pooling), 197 of
    the ViT ([CLS] and the patches), for ``--sketch_attn tokens``."""
    st = getattr(args, 'sketch_tokens', None) or 'pooled'
    if st not in SKETCH_TOKENS:
        raise ValueError(f'args.sketch_tokens must be one of {SKETCH_TOKENS}, not {st!r}')
    return st


def _resnet_backbone(args, video_net, sketch_net, width, sk):
    """the ResNet pair of either depth: sets both input widths, reads --train_backbone / --freeze_backbone / --sync_bn / --compute_dtype"""
    from .resnet import ResNetBackbone
    args.input_vid_dim = width
    args.input_skch_dim = width
    cd = getattr(args, 'compute_dtype', 'bf16')
    # the torchvision IMAGENET1K_V1 weights are loaded by the caller (load_state_dict with the reference's backbone.* keys) —
    # nothing is downloaded here.  The reference TRAINS its backbone: train.py:72 hands every parameter of build_model(args) to
    # the optimiser and model.train() puts BatchNorm into batch-statistics mode (its --freeze_backbone flag is parsed and never
    # read).  So a reference-style run gets the trainable extractors (csrc/resnet_train.hip) by default; --freeze_backbone — dead
    # in the reference, honoured here — or --train_backbone 0 selects the frozen, BatchNorm-folded extractors (inference, or the
    # features-are-fixed setting bench.py --workload resnet measures without --train-backbone).
    tb = getattr(args, 'train_backbone', None)
    tb = (not bool(getattr(args, 'freeze_backbone', False))) if tb is None else bool(tb)
    sync = bool(getattr(args, 'sync_bn', False))   # train.py:65-68: apex convert_syncbn_model
    return ResNetBackbone(video_net(compute_dtype=cd, trainable=tb, sync_bn=sync),
                          sketch_net(avgpool=_sketch_tokens(args) == 'pooled', compute_dtype=cd, trainable=tb, sync_bn=sync),
                          pixel_preset=getattr(args, 'pixel_preset', None), **sk)


def build_backbone(args):
    """Like backbone.py:116-152 this MUTATES args (input_vid_dim / input_skch_dim).  ``args.compute_dtype`` goes to the extractors: the
    ViT pair takes fp16 and otherwise stays bf16 (module docstring); the ResNet pair takes it as it is — bf16, fp16 (frozen and
    trainable; what the reference's apex amp runs) or fp32 (frozen only) — so a bf16 or fp32 head keeps the extractors it always had."""
    if args.backbone == 'features':
        args.input_vid_dim = getattr(args, 'input_vid_dim', 512)
        args.input_skch_dim = getattr(args, 'input_skch_dim', 512)
        return FeatureBackbone()
    # the sketch's own ingest (svol_amd/ingest.py): set on the args object like pixel_preset, no command-line flag
    sk = dict(sketch_filter=getattr(args, 'sketch_filter', None), sketch_invert=bool(getattr(args, 'sketch_invert', False)))
    if 'vit' in args.backbone:  # backbone.py:117-132: ViT-B/16 for frames and sketch, 768-wide features
        from .backbone import ViTBackbone, ViTExtractor, vit_base_config
        args.input_vid_dim = 768
        args.input_skch_dim = 768
        # the pretrained google/vit-base-patch16-224-in21k weights are loaded by the caller
        # (ViTExtractor.load_hf_state_dict); nothing is downloaded here.  Trained only on an explicit --train_backbone 1 (module
        # docstring: why the default differs from the ResNet's)
        tb = bool(getattr(args, 'train_backbone', None) or False)
        tl = getattr(args, 'finetune_layers', None) if tb else None
        cd = 'fp16' if getattr(args, 'compute_dtype', 'bf16') == 'fp16' else 'bf16'   # (module docstring)
        return ViTBackbone(ViTExtractor(vit_base_config(), compute_dtype=cd, trainable=tb, train_layers=tl),
                           ViTExtractor(vit_base_config(), compute_dtype=cd, trainable=tb, train_layers=tl),
                           pixel_preset=getattr(args, 'pixel_preset', None), sketch_tokens=_sketch_tokens(args), **sk)
    if args.backbone == 'resnet50':  # backbone.py:143-147: ResNet-50 on the frames and, average-pooled, on the sketch; 2048-wide features
        from .resnet import resnet50
        return _resnet_backbone(args, resnet50, resnet50, 2048, sk)
    if 'resnet' in args.backbone:  # backbone.py:133-152: ResNet-34 on the frames (7x7 tokens), ResNet-18 + avgpool on the sketch
        from .resnet import resnet18, resnet34
        return _resnet_backbone(args, resnet34, resnet18, 512, sk)
    raise NotImplementedError(f"backbone '{args.backbone}' is not part of the MI355X build (the reference has it commented out)")


class SketchLocalizationModel(nn.Module):
    def __init__(self, backbone, head):
        super().__init__()
        self.backbone = backbone
        self.head = head

    def forward(self, src_sketch, src_video, src_sketch_mask=None, src_video_mask=None):
        # raw uint8 frames may come as a list of B tensors [T, H_b, W_b, 3] (svol_amd/ingest.py): T is then the first one's length
        T = src_video[0].shape[0] if isinstance(src_video, (list, tuple)) else src_video.shape[1]
        src_sketch, src_video = self.backbone(src_sketch, src_video)
        # per-token masks: one sketch-mask entry per sketch token, one frame-mask entry per patch (model.py:21-22)
        # (n sketches, --num_input_sketches: a [B, n] mask over n * tokens sketch tokens; with one column the factor is what it always was)
        src_sketch_mask = src_sketch_mask.repeat_interleave(src_sketch.shape[1] // src_sketch_mask.shape[1], dim=1)
        src_video_mask = src_video_mask.repeat_interleave(src_video.shape[1] // T, dim=1)
        return self.head(src_sketch, src_sketch_mask, src_video, src_video_mask)


def build_model(args):
    backbone = build_backbone(args)
    if args.sketch_head == 'svanet':
        head = build_svanet(args)
    elif args.sketch_head == 'sketch_detr':  # model.py:35-36; needs the build's --enc_layers/--dec_layers/--mode/--feat_dim
        from .sketch_detr import build_sketchdetr
        head = build_sketchdetr(args)
    elif args.sketch_head == 'svanet_variants':  # the reference's svanet_variants.py has no dispatch entry of its own
        from .svanet_variants import build_svanet as build_svanet_variants
        head = build_svanet_variants(args)
    else:
        raise NotImplementedError
    return SketchLocalizationModel(backbone, head)
