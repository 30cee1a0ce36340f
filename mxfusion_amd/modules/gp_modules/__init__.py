from .gp_regression import GPRegression  # noqa: F401
from .svgp_regression import SVGPRegression  # noqa: F401
from .sparsegp_regression import SparseGPRegression  # noqa: F401
from .likelihoods import BernoulliLogit, BernoulliProbit, PoissonExp, RobustMax  # noqa: F401
from .svgp_likelihood import SVGPLikelihood  # noqa: F401
from .bayesian_gplvm import BayesianGPLVM, BayesianGPLVMUncertainInputPrediction  # noqa: F401
from .pathwise import (GPRegressionPathwiseSampling, SVGPRegressionPathwiseSampling, SparseGPRegressionPathwiseSampling,  # noqa: F401
                       PathwiseSamples)
from .iterative_gp_regression import (IterativeGPRegression, IterativeGPRegressionLogPdf,  # noqa: F401
                                       IterativeGPRegressionMeanVariancePrediction)
from .vecchia_gp_regression import (VecchiaGPRegression, VecchiaGPRegressionLogPdf,  # noqa: F401
                                     VecchiaGPRegressionMeanVariancePrediction)
