"""GPU counterparts of the reference's scoring stage: score/prob_inference.py (per-frame
view-mean probabilities) and score/sv_level/LiDAL.py (inter-frame divergence / entropy per
supervoxel + greedy selection), with frames sharded over the GPUs of a node; and the ReDAL baseline
(score/sv_level/ReDAL.py: surface variation, region scores, k-means, diversity-aware selection) on one GPU; and the
frame-level baselines (score/frame_level/: entropy, margin, confidence, segment entropy, core-set, random); and, beyond
the reference, the disagreement of a frame's own augmented views per supervoxel and per frame (view_level.py), and
annotations and predictions carried across the registered frames of a sequence (transfer.py), and the poses themselves
for sequences that come without: scan-to-scan point-to-plane ICP (registration.py); and the MC-dropout baseline per
supervoxel and per frame (mc_dropout.py)."""
from .frame_level import (FrameBoard, coreset, frame_feature, frame_sequence, frame_uncertainty, random_frames,
                          segment_entropy, select_frames)
from .interframe import FrameBank, neighbour_ids, score_frame
from .pipeline import ScoreBoard, collect_sequence, score_sequence
from .mc_dropout import frame_mc_scores, mc_sequence
from .prob_inference import infer_frame, mc_scores
from .registration import IcpTarget, icp, point_normals, register_sequence
from .redal import (RegionBoard, kmeans, knn, redal_sequence, region_scores, select_redal,
                    surface_variation)
from .selection import centre_pairs, select, select_indexed
from .sharding import HaloExchange, frame_range, gather_frames, needed_frames
from .transfer import fuse_predictions, match_points, transfer_labels, transfer_sequence
from .view_level import frame_view_scores, score_frame_views, view_sequence

__all__ = ['infer_frame', 'FrameBank', 'neighbour_ids', 'score_frame', 'score_sequence', 'collect_sequence', 'ScoreBoard', 'select',
           'select_indexed', 'centre_pairs',
           'frame_range', 'gather_frames', 'needed_frames', 'HaloExchange',
           'surface_variation', 'knn', 'region_scores', 'kmeans', 'select_redal', 'RegionBoard', 'redal_sequence',
           'frame_uncertainty', 'segment_entropy', 'frame_feature', 'coreset', 'select_frames', 'random_frames',
           'frame_sequence', 'FrameBoard', 'score_frame_views', 'frame_view_scores', 'view_sequence',
           'match_points', 'transfer_labels', 'fuse_predictions', 'transfer_sequence',
           'point_normals', 'IcpTarget', 'icp', 'register_sequence', 'mc_scores', 'mc_sequence', 'frame_mc_scores']
