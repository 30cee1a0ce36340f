from .distribution import Distribution  # noqa: F401
from .normal import Normal, NormalMeanPrecision  # noqa: F401
from .pointmass import PointMass  # noqa: F401
from .univariate import UnivariateDistribution  # noqa: F401
from .gamma import Gamma, GammaMeanVariance  # noqa: F401
from .beta import Beta  # noqa: F401
from .laplace import Laplace  # noqa: F401
from .uniform import Uniform  # noqa: F401
from .mvn import MultivariateNormal, MultivariateNormalMeanPrecision  # noqa: F401
from .wishart import Wishart  # noqa: F401
from .categorical import Categorical  # noqa: F401
from .dirichlet import Dirichlet  # noqa: F401
from .bernoulli import Bernoulli  # noqa: F401
from .random_gen import RandomGenerator, TorchRandomGenerator, MockRandomGenerator  # noqa: F401
from .gp import GaussianProcess, ConditionalGaussianProcess  # noqa: F401
