"""hint_amd — MI355X-native (gfx950) implementation of HINT's recursive affine-coupling block.

Public surface mirrors /root/reference/hint.py (see hint_amd/hint.py); the compute lives in
hint_amd/csrc behind the C ABI of include/hint_amd.h.
"""
from .hint import (HierarchicalAffineCouplingBlock, HierarchicalAffineCouplingTree,  # noqa: F401
                   HintAmdError, linear_subnet_constructor, set_pack_cache, set_param_grad_mode)

from .flow import FixedOrthogonal, HintFlow  # noqa: F401,E402
from .householder import HouseholderPerm  # noqa: F401,E402
from .train import FlowTrainer  # noqa: F401,E402
from .conditional import (AffineCoupling, ConditionalFlowTrainer, ConditionalHintFlow,  # noqa: F401,E402
                          ExternalAffineCoupling, F_fully_connected)
from .optim import ClampAdam  # noqa: F401,E402
from .metrics import MultiMMD, multi_mmd  # noqa: F401,E402
from .metrics import CorrelationTarget, corr_mse, corrcoef  # noqa: F401,E402
from .abc import nearest_rows, quantile_abc  # noqa: F401,E402
from .curves import curve_features, lens_forward_process, mean_target_distance, target_distances  # noqa: F401,E402
from .curves import chamfer_distances, hausdorff_distances, lens_fit_loss, trace_fourier_curves  # noqa: F401,E402
from .curves import (plus_fit_loss, plus_fit_terms, plus_hausdorff_distances, plus_outline_counts,  # noqa: F401,E402
                     plus_segments)
from .curves import fit_lens_shapes, lens_fit_grad, lens_fit_starts  # noqa: F401,E402
from .curves import fit_plus_shapes, plus_dominant_angle, plus_fit_grad, plus_fit_starts  # noqa: F401,E402
from .curves import (lens_iou_dice, lens_shape_scores, plus_iou_dice, plus_shape_scores,  # noqa: F401,E402
                     polygon_overlap)
from .shapes import fourier_coeffs, lens_draws, lens_rings, sample_lens_joint, sample_lens_prior  # noqa: F401,E402
from .plusgen import (plus_draws, plus_outlines, sample_plus_conditional, sample_plus_joint,  # noqa: F401,E402
                      sample_plus_prior, sample_plus_targeted)
from .data import DeviceDataset, epoch_indices, reference_lr  # noqa: F401,E402

__version__ = "0.1.0"
