"""GPU counterparts of the reference's scoring stage: score/prob_inference.py (per-frame
view-mean probabilities) and score/sv_level/LiDAL.py (inter-frame divergence / entropy per
supervoxel + greedy selection), with frames sharded over the GPUs of a node; and the ReDAL baseline
(score/sv_level/ReDAL.py: surface variation, region scores, k-means, diversity-aware selection) on one GPU."""
from .interframe import FrameBank, neighbour_ids, score_frame
from .pipeline import ScoreBoard, collect_sequence, score_sequence
from .prob_inference import infer_frame
from .redal import (RegionBoard, kmeans, knn, redal_sequence, region_scores, select_redal,
                    surface_variation)
from .selection import select
from .sharding import HaloExchange, frame_range, gather_frames, needed_frames

__all__ = ['infer_frame', 'FrameBank', 'neighbour_ids', 'score_frame', 'score_sequence', 'collect_sequence', 'ScoreBoard', 'select',
           'frame_range', 'gather_frames', 'needed_frames', 'HaloExchange',
           'surface_variation', 'knn', 'region_scores', 'kmeans', 'select_redal', 'RegionBoard', 'redal_sequence']
