"""yolo_dual_amd — MI355X-native (gfx950) segmentation training hot path behind the reference's module API.

Public surface mirrors the reference's seg scripts and models/common.py (names, constructor signatures, state_dict
layout).  All compute runs in hand-written HIP kernels (libydl_hip.so, C ABI in include/ydl.h); there is no CPU or
ATen fallback — importing is cheap, the first GPU call loads the library and fails loudly if it was not built."""
from . import config
from .config import compute_dtype, set_compute_dtype
from .checkpoint import (fuse_conv_and_bn, intersect_dicts, load_checkpoint, load_weights, save_checkpoint, smart_resume,
                         strip_optimizer)
from .data import AugmentGPU, LetterboxGPU, draw_augmentations, letterbox_geometry
from .evaluate import ConfusionMatrix
from .loss import JaccardSegmentationLoss, SegmentationLoss
from .models import (ResNet18, ResNet18Seg, ResNet50, ResNet50Seg, ResNet50SegYaml, SegYoloModel, YOLOv5Seg, YOLOv8Seg,
                     YOLOv9Seg, default_activation, parse_model, resolve_activation)
from .modules import (GAM, AttentionConv, AttentionStem, C2f, C3, C3k2, C3_DCNV3, BasicBlock, Bottleneck, Bottleneck_DCNV3, BottleneckBlock, C3Common, Concat,
                      Conv, C2f_DCN, C3_DCN, C3_DCNCommon, Bottleneck_DCN, DCNv2, DCNv3, DCNV3_YoLo, DeformConv2d, Linear, MaxPool2d, SegmentHead, SPPF, Upsample, autopad,
                      C3Ghost, DWConv, GhostBottleneck, GhostConv, C3TR, TransformerBlock, TransformerLayer, ASPP, RFB, BasicConv,
                      SPP, C3SPP, SimConv, SimSPPF, SPPCSPC, SPPCSPC_group, SimCSPSPPF, CrossConv, C3x, ConvTranspose2d, DWConvTranspose2d,
                      Focus, Contract, Expand, BottleneckCSP, BatchNorm2d,
                      LayerNorm2d, CNBlock, convnext_tiny1, convnext_tiny2, convnext_tiny3, convnext_key_map,
                      SqueezeExcitation, Conv2dNormActivation, InvertedResidual, MBConv, MobileNetV3s1, MobileNetV3s2, MobileNetV3s3,
                      efficientnet_b01, efficientnet_b02, efficientnet_b03, mobilenet_v3_small_key_map, efficientnet_b0_key_map)
from .deform import deform_conv2d
from . import activations
from .activations import AconC, FReLU, Hardswish, MemoryEfficientMish, MetaAconC, Mish, SiLU
from . import predict
from .predict import (SegmentationMetrics, argmax_labels, colorize, default_palette, difference, label_class_weights, overlay,
                      predict_labels, unletterbox_labels)
from .optim import FlatAdamEMA, FlatAdamWEMA, FlatArenaOptimizer, FlatRMSPropEMA, FlatSGDEMA, smart_optimizer

__all__ = [n for n in dir() if not n.startswith("_")]
