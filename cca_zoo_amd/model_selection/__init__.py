"""Model selection for multiview models (surface of cca_zoo/model_selection/__init__.py), permutation, bootstrap and jackknife
inference."""

from cca_zoo_amd.model_selection._bootstrap import BCaBootstrapResult, BootstrapResult, bootstrap
from cca_zoo_amd.model_selection._jackknife import JackknifeResult, bca_intervals, jackknife
from cca_zoo_amd.model_selection._permutation import PermutationTestResult, permutation_test
from cca_zoo_amd.model_selection._search import GridSearchCV

__all__ = ["GridSearchCV", "permutation_test", "PermutationTestResult", "bootstrap", "BootstrapResult", "BCaBootstrapResult",
           "jackknife", "JackknifeResult", "bca_intervals"]
