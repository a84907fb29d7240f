"""Model selection for multiview models (surface of cca_zoo/model_selection/__init__.py), permutation and bootstrap inference."""

from cca_zoo_amd.model_selection._bootstrap import BootstrapResult, bootstrap
from cca_zoo_amd.model_selection._permutation import PermutationTestResult, permutation_test
from cca_zoo_amd.model_selection._search import GridSearchCV

__all__ = ["GridSearchCV", "permutation_test", "PermutationTestResult", "bootstrap", "BootstrapResult"]
