from .function_evaluation import FunctionEvaluation, MXFusionFunction  # noqa: F401
from .torch_function import MXFusionTorchFunction, MXFusionGluonFunction, TorchFunctionEvaluation, GluonFunctionEvaluation  # noqa: F401
