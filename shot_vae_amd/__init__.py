"""shot_vae_amd: MI355X-native (gfx950 HIP) implementation of the SHOT-VAE training hot path behind
the reference's Python API (FengHZ/SHOT-VAE: shot_vae_model/vae.py, lib/criterion.py,
lib/utils/mixup.py, the step of main_shot_vae.py)."""
from .vae import VariationalAutoEncoder, Scores  # noqa: F401
from .criterion import VAECriterion, ClsCriterion, continuous_posterior_loss   # noqa: F401
from .mixup import mixup_vae_data, label_smoothing, optimal_match_index        # noqa: F401
from .optim import FlatSGD, FlatAdam              # noqa: F401
from .train import (train_step, train_step_overlapped, train_step_grouped, GraphedTrainStep, DeviceRng, schedule,   # noqa: F401
                    alpha_schedule, m2_train_step, apply_update, inference_kl)
from .evaluate import (Evaluator, evaluate, evaluate_scores, SmoothEvaluator, evaluate_smooth, KnnEvaluator,       # noqa: F401
                       evaluate_knn)
from .classifier import (WideResNetClassifier, get_wide_resnet, CrossEntropyLoss, classifier_train_step,      # noqa: F401
                         GraphedClassifierStep, ClassifierEvaluator, evaluate_classifier)
from .data import DeviceDataset, ssl_split      # noqa: F401
from .smooth import (SmoothVAE, svhn_VAE, mnist_VAE, SmoothELBOLoss, smooth_train_step,      # noqa: F401
                     GraphedSmoothStep)
from .neighbors import (LatentIndex, encode_posterior, pairwise_distance, pairwise_norm_kl_dist_gpu,      # noqa: F401
                        pairwise_square_euclidean_gpu, pairwise_norm_wasserstein_dist_gpu, calculate_mean_dist_pairwise)
from .aggregate import AggregatePosterior, evaluate_aggregate      # noqa: F401
from .quality import (Manifold, manifold_metrics, FeatureMoments, frechet_distance, evaluate_generation)      # noqa: F401
from .cluster import (KMeans, kmeans_plus_plus, contingency, linear_assignment, partition_metrics,      # noqa: F401
                      evaluate_clustering)
from .calibration import (row_stats, Reliability, TemperatureScaler, rank_counts, detection_metrics,      # noqa: F401
                          selective_metrics, evaluate_calibration, evaluate_detection)
from .embed import TSNE, conditional_affinities, symmetrize, pca_project, evaluate_embedding      # noqa: F401
from .mixture import GaussianMixture, evaluate_mixture, generate_from_mixture      # noqa: F401
from .probe import LinearProbe, evaluate_probe, select_labels      # noqa: F401
from .propagate import LabelPropagator, knn_graph, normalize_graph, evaluate_propagation      # noqa: F401
from .twosample import (kernel_sums, median_bandwidth, mmd2, witness, kid, permutation_test, evaluate_two_sample,      # noqa: F401
                        evaluate_prior_match, evaluate_kid)
from .validity import (silhouette_grouped, silhouette_samples, silhouette_score, cluster_spread, calinski_harabasz,      # noqa: F401
                       davies_bouldin, validity_indices, evaluate_validity)
from .trace import StepLogger, step_range, enable_ranges     # noqa: F401
