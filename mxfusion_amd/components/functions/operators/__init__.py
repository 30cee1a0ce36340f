from .operators import Operator, OperatorDecorator, MXNetOperatorDecorator, BroadcastToOperator  # noqa: F401
from .operators import (add, subtract, multiply, divide, power, square, exp, log, sum, mean, prod, dot, diag, reshape, transpose,  # noqa: F401
                        broadcast_to)
