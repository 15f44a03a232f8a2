"""sibrar---single-branch-recommender_amd — MI355X (gfx950) engine for the SiBraR SingleBranchNet hot path.

Hand-written HIP kernels behind a C ABI (include/sibrar_hip.h, csrc/), driven through the reference's own plugin surface:
``SingleBranchNet`` / ``SGDBaseline`` (SGDBasedRecommenderAlgorithm), the ``RecommenderSystemLoss`` classes, ``Trainer`` and
``evaluate_recommender_algorithm`` / ``FullEvaluator``. Import as ``import sibrar_amd`` (root-level shim) or through
``importlib.import_module('sibrar---single-branch-recommender_amd')``.
"""
from ._lib import SibrarHipError, lib, LIB_PATH                                            # noqa: F401
from .config import (DropoutNetConfig, DropoutNetEntityConfig, DropoutNetSamplingStrategy,   # noqa: F401
                     EmbeddingRegularizationType, FeatureModuleConfig, SingleBranchFeatureConfig,
                     SingleBranchNetConfig, SingleBranchNetEntityConfig)
from .features import DeviceTable, HostFeature                                              # noqa: F401
from .polylinear import PolyLinear                                                          # noqa: F401
from .sbnet import (FeatureEmbedding, ItemFeatureMatrixFactorization, SGDBasedRecommenderAlgorithm, SGDBaseline,   # noqa: F401
                    SGDMatrixFactorization, SingleBranchNet, SingleBranchNetEntity, UserFeatureMatrixFactorization,
                    general_weight_init)
from .dropoutnet import DropoutNet, DropoutNetEntity                                      # noqa: F401
from .deepmf import DeepMatrixFactorization                                                # noqa: F401
from .protomf import IProtoMF, PrototypeWrapper, UIProtoMF, UProtoMF                       # noqa: F401
from .protomfs import IProtoMFs, UIProtoMFs, UIProtoMFsCombine, UProtoMFs                   # noqa: F401
from .acf import ACF                                                                        # noqa: F401
from .ecf import ECF, ecf_tag_matrix                                                        # noqa: F401
from .matrix_models import FactorModel, ResidentMatrixAlgorithm, SparseMatrixBasedRecommenderAlgorithm   # noqa: F401
from .knn import ItemFeatureKNN, ItemKNN, KNNAlgorithm, SimilarityFunctionEnum, UserKNN                     # noqa: F401
from .ease import EASE                                                                      # noqa: F401
from .slim import SLIM                                                                      # noqa: F401
from .p3alpha import P3alpha                                                                # noqa: F401
from .lightgcn import LightGCN                                                              # noqa: F401
from .multvae import MultDAE, MultVAE                                                       # noqa: F401
from .recvae import RecVAE                                                                  # noqa: F401
from .directau import DirectAU                                                              # noqa: F401
from .simgcl import SimGCL, XSimGCL                                                         # noqa: F401
from .ultragcn import UltraGCN                                                              # noqa: F401
from .simplex import SimpleX                                                                # noqa: F401
from .neumf import NeuMF                                                                    # noqa: F401
from .ngcf import NGCF                                                                      # noqa: F401
from .als import AlternatingLeastSquare                                                     # noqa: F401
from .svd import SVDAlgorithm                                                               # noqa: F401
from .rbmf import RBMF                                                                      # noqa: F401
from .naive import PopularItems, RandomItems                                                # noqa: F401
from .losses import (InfoNCE, RecAlignmentLoss, RecBayesianPersonalizedRankingLoss, RecBinaryCrossEntropy, RecNoLoss,   # noqa: F401
                     RecSampledSoftmaxLoss, RecommenderSystemLoss, RecommenderSystemLossesEnum)
from .optim import FlatParameters, FusedOptimizer                                           # noqa: F401
from .trainer import Trainer                                                                # noqa: F401
from .engine import FusedTrainStep                                                          # noqa: F401
from .evaluation import (FullEvaluator, Gatherer, evaluate_recommender_algorithm, gather_recommender_algorithm_results,   # noqa: F401
                         paired_significance)
from .datasets import NegativeSamplingDataLoader, SyntheticDataset                          # noqa: F401
from .splitdata import SplitDataset, load_split_dataset                                     # noqa: F401
from . import ops, parallel, sampling                                                       # noqa: F401


def reproducible(seed: int, deterministic: bool = True) -> None:
    """utilities/utils.py:22-27 (``reproducible(seed)``): seeds Python's, NumPy's and torch's generators and switches the engine's
    deterministic mode on (``ops.set_deterministic``) — the counterpart of ``torch.backends.cudnn.deterministic = True``: the same
    seed then gives the same model, bit for bit, on one GPU."""
    import random
    import numpy as np
    import torch
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    ops.set_deterministic(deterministic)

# the reference's registry: AlgorithmsEnum.sbnet / .sgdbias / .mf / .dmf / .uprotomf / .iprotomf / .uiprotomf / .uprotomfs / .iprotomfs /
# .uiprotomfs / .acf / .ecf / .uknn / .iknn / .ifknn / .ease / .slim / .p3alpha / .als / .svd / .rbmf / .pop / .rand -> class
# (algorithms/algorithms_utils.py); 'lightgcn', 'multvae', 'multdae', 'recvae', 'directau', 'simgcl', 'xsimgcl', 'ultragcn', 'simplex', 'neumf' and 'ngcf' are this package's own: the reference has
# no trained graph model, no autoencoder over the interaction row, no model trained on alignment and uniformity, no contrastive one and
# none whose score is a learned non-linear function of the pair ('ngcf' is the graph model with weights in its layers that 'lightgcn'
# simplifies)
ALGORITHMS = {'sbnet': SingleBranchNet, 'sgdbias': SGDBaseline, 'mf': SGDMatrixFactorization,
              'ifeatmf': ItemFeatureMatrixFactorization, 'ufeatmf': UserFeatureMatrixFactorization, 'dropoutnet': DropoutNet, 'dmf': DeepMatrixFactorization,
              'uprotomf': UProtoMF, 'iprotomf': IProtoMF, 'uiprotomf': UIProtoMF, 'uprotomfs': UProtoMFs, 'iprotomfs': IProtoMFs,
              'uiprotomfs': UIProtoMFs, 'acf': ACF, 'ecf': ECF, 'uknn': UserKNN, 'iknn': ItemKNN, 'ifknn': ItemFeatureKNN, 'ease': EASE,
              'slim': SLIM, 'p3alpha': P3alpha, 'als': AlternatingLeastSquare, 'svd': SVDAlgorithm, 'rbmf': RBMF,
              'pop': PopularItems, 'rand': RandomItems, 'lightgcn': LightGCN, 'multvae': MultVAE, 'multdae': MultDAE, 'recvae': RecVAE,
              'directau': DirectAU, 'simgcl': SimGCL, 'xsimgcl': XSimGCL, 'ultragcn': UltraGCN, 'simplex': SimpleX,
              'neumf': NeuMF, 'ngcf': NGCF}
