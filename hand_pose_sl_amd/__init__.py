"""hand_pose_sl_amd -- MI355X-native body->hand keypoint inference path.

A from-scratch gfx950 implementation of the one convolutional model of
benoriol/hand_pose_sl (`ConvModel`, body2hand/src/models/HandPoseModels.py:17-64)
behind the reference's own call surface.  See DESIGN.md and include/b2h.h.
"""
from .conv_model import ConvModel, LinearPositionalEmbedding, target_transform  # noqa: F401
from .dataset import Augment, DeviceDataset, DeviceLoader  # noqa: F401
from .evaluate import train_epoch, validate  # noqa: F401
from .graph_trainer import GraphTrainer  # noqa: F401
from .metrics import l1_to_pixels, masked_pose_l1, maskedPoseL1, poderatedPoseL1, weighted_pose_l1  # noqa: F401
from .optim import Adam  # noqa: F401
from .padding import token_lengths  # noqa: F401
from .predict import joint_pixel_error, predict_dataset, window_plan  # noqa: F401
from .text_pose_transformer import TextPoseTransformer  # noqa: F401
from .transformer_enc import PositionalEncoding, TransformerEnc  # noqa: F401

__all__ = ["ConvModel", "LinearPositionalEmbedding", "target_transform", "masked_pose_l1", "weighted_pose_l1",
           "l1_to_pixels", "maskedPoseL1", "poderatedPoseL1", "validate", "TransformerEnc", "PositionalEncoding",
           "TextPoseTransformer", "Adam", "DeviceDataset", "DeviceLoader", "Augment", "train_epoch",
           "GraphTrainer", "window_plan", "predict_dataset", "joint_pixel_error", "token_lengths"]
