from .pose_metrics import BasicKeyPointDecoder, GaussTaylorKeyPointDecoder  # noqa: F401
from .pose_metrics import evaluate_map  # noqa: F401
from .coco_eval import KeypointEvaluator, KeypointGroundTruth  # noqa: F401
from .flip import COCO_JOINT_PAIRS, merge_flipped, mirror_input, pairs_to_perm  # noqa: F401
