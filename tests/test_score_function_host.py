"""Host checks of the score-function feature: the constructor signatures against the reference's (mxfusion/inference/score_function.py:43,
:107: num_samples, model, posterior, observed; `baseline` is this project's addition, last and optional) and FactorGraph.get_descendants /
get_markov_blanket (factor_graph.py:331-357) on a three-level graph."""
import inspect


def test_constructor_argument_names_match_the_reference():
    from mxfusion_amd.inference import ScoreFunctionInference, ScoreFunctionRBInference, StochasticVariationalInference
    for cls in (ScoreFunctionInference, ScoreFunctionRBInference):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names == ['self', 'num_samples', 'model', 'posterior', 'observed', 'baseline'], names
        assert inspect.signature(cls.__init__).parameters['baseline'].default is None
        assert issubclass(cls, StochasticVariationalInference)
    assert issubclass(ScoreFunctionRBInference, ScoreFunctionInference)


def _three_levels():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import Normal
    m = Model()
    m.s = Variable(shape=(1,))
    m.a = Normal.define_variable(mean=0., variance=m.s, shape=(1,))
    m.b = Normal.define_variable(mean=m.a, variance=1., shape=(1,))
    m.c = Normal.define_variable(mean=m.a + m.b, variance=1., shape=(1,))
    m.d = Normal.define_variable(mean=0., variance=1., shape=(1,))
    return m


def test_get_descendants_on_a_three_level_graph():
    m = _three_levels()
    total = m.c.factor.inputs[0][1]                         # the function variable a + b
    assert m.get_descendants(m.c) == {m.c}
    assert m.get_descendants(m.b) == {m.b, total, m.c}
    assert m.get_descendants(m.a) == {m.a, m.b, total, m.c}
    assert m.get_descendants(m.s) == {m.s, m.a, m.b, total, m.c}
    assert m.get_descendants(m.d) == {m.d}


def test_get_markov_blanket():
    m = _three_levels()
    total = m.c.factor.inputs[0][1]
    zero, one = (v for _, v in m.a.factor.inputs if v is not m.s).__next__(), m.b.factor.inputs[1][1]
    assert m.get_markov_blanket(m.a) == {m.a, zero, m.s, m.b, one, total}
    assert m.get_markov_blanket(m.c) == {m.c, total, m.c.factor.inputs[1][1]}
