"""Circuits, inputs and (cached) float64 oracle results for the posterior queries of node-graph SPNs (test helper).

Every circuit gets ONE input block of 257 rows, of which the batch sizes under test are prefixes (a row's result depends on
the row alone): rows drawn by tests/flat_spn_query_cases.py::support_inputs with NaN rates 0, 0.5 and 1 and shuffled, so
that every prefix mixes the rates; row 0 all NaN; rows 1 .. 3 carry evidence of probability zero; three extra columns
behind the circuit's features (all NaN, a constant, a mix of NaN and finite values)."""
import functools
import json
import os

import numpy as np

from tests import flat_spn_posterior_ref as pref
from tests.flat_spn_cases import random_circuit
from tests.flat_spn_query_cases import support_inputs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROWS = 257
BATCHES = (1, 63, 64, 65, 257)
EXTRA = 3
CIRCUITS = ('binary16', 'mixed4', 'random5', 'random5_small', 'random12', 'random17', 'shared')
# name -> random_circuit(n_features, seed, n_sum).  Every sum node over several variables has n_sum >= 2 product children,
# so a moment or a posterior depends on the evidence about the other variables, and every circuit has all four leaf
# families.  Nodes: 382 / 121 / 976 / 1666; only random5_small fits the on-chip route (128 nodes).  (The default of three
# products per sum node gives 35689 nodes at 12 variables, on which the float64 oracle -- one forward pass per
# variable -- takes minutes; two per sum node keep 12 and 17 variables at a size it handles in seconds.)
RANDOM = {'random5': (5, 2, 3), 'random5_small': (5, 3, 2), 'random12': (12, 5, 2), 'random17': (17, 0, 2)}
ON_CHIP = {'binary16': True, 'mixed4': True, 'shared': True, 'random5_small': True, 'random5': False, 'random12': False,
           'random17': False}


def shared_child_circuit():
    """A product node (#5) that is the child of two different sum nodes (#3, #4): its gradient row accumulates from two
    parents.  Variable 0 Bernoulli, 1 Gaussian, 2 Categorical whose category 2 has probability zero under both leaves."""
    nodes, links = [], []

    def new(cls, scope, **attrs):
        nodes.append(dict({'id': len(nodes), 'class': cls, 'scope': scope}, **attrs))
        return len(nodes) - 1

    def link(parent, kids):
        for idx, c in enumerate(kids):
            links.append({'source': c, 'target': parent, 'idx': idx})

    root = new('Sum', [0, 1, 2], weights=[0.35, 0.65])
    t1, t2 = new('Product', [0, 1, 2]), new('Product', [0, 1, 2])
    sa, sb = new('Sum', [0, 1], weights=[0.25, 0.75]), new('Sum', [0, 1], weights=[0.6, 0.4])
    p, q1, q2 = (new('Product', [0, 1]) for _ in range(3))
    bern = [new('Bernoulli', [0], params={'p': v}) for v in (0.2, 0.7, 0.9)]
    gauss = [new('Gaussian', [1], params={'mean': m, 'stddev': s}) for m, s in ((-1.0, 0.5), (0.5, 1.5), (2.0, 0.8))]
    cats = [new('Categorical', [2], params={'categories': [0, 1, 2, 3], 'probabilities': pr})
            for pr in ([0.5, 0.25, 0.0, 0.25], [0.125, 0.5, 0.0, 0.375])]
    link(root, [t1, t2])
    link(t1, [sa, cats[0]])
    link(t2, [sb, cats[1]])
    link(sa, [p, q1])
    link(sb, [p, q2])
    for prod, k in ((p, 0), (q1, 1), (q2, 2)):
        link(prod, [bern[k], gauss[k]])
    d = {'directed': True, 'multigraph': False, 'graph': {}, 'nodes': nodes, 'links': links}
    return d, ['Bernoulli', 'Gaussian', 'Categorical']


@functools.lru_cache(maxsize=None)
def circuit(name):
    """(json dict, leaf family per variable)."""
    if name == 'shared':
        return shared_child_circuit()
    if name in RANDOM:
        n, seed, n_sum = RANDOM[name]
        return random_circuit(n, seed, n_sum=n_sum)
    with open(os.path.join(GOLD, 'spn_%s.json' % name)) as f:
        d = json.load(f)
    family = {}
    for n in d['nodes']:
        if n['class'] in pref.LEAVES:
            family[int(n['scope'][0])] = n['class']
    return d, [family[v] for v in range(len(family))]


def _zero_probability_value(name, family):
    """(variable, value): an observation no leaf over the variable gives a positive probability."""
    if name == 'shared':
        return 2, 2.0                   # the category both leaves give probability zero
    for v, f in enumerate(family):
        if f == 'Categorical':
            return v, 7.0               # outside every leaf's categories
    for v, f in enumerate(family):
        if f == 'Uniform':
            return v, 1e3               # outside every leaf's interval
    return 0, 2.0                       # a Bernoulli variable observed at neither 0 nor 1


@functools.lru_cache(maxsize=None)
def inputs(name):
    """[ROWS, n_features + EXTRA] float32 (treat as read-only)."""
    d, family = circuit(name)
    D = len(family)
    seed = 1000 + CIRCUITS.index(name)
    parts = [support_inputs(d, family, n, seed + k, rate) for k, (n, rate) in enumerate(((86, 0.0), (86, 0.5), (85, 1.0)))]
    x = np.concatenate(parts)[np.random.RandomState(seed).permutation(ROWS)]
    rs = np.random.RandomState(seed + 7)
    x[0] = np.nan
    var, value = _zero_probability_value(name, family)
    for r, rate in ((1, 1.0), (2, 0.5), (3, 0.0)):
        fill = parts[0][r + 10].copy()
        fill[rs.rand(D) < rate] = np.nan
        x[r] = fill
        x[r, var] = value
    wide = np.full((ROWS, D + EXTRA), np.nan, np.float32)
    wide[:, :D] = x
    wide[:, D + 1] = 3.25
    wide[:, D + 2] = np.where(rs.rand(ROWS) < 0.5, np.nan, rs.randn(ROWS)).astype(np.float32)
    wide.setflags(write=False)
    return wide


@functools.lru_cache(maxsize=None)
def oracle(name):
    return pref.Oracle(circuit(name)[0])


@functools.lru_cache(maxsize=None)
def oracle_moments(name):
    """(want, scale) [4, ROWS, D + EXTRA] float64 (treat as read-only)."""
    want, scale = oracle(name).moments(inputs(name), 4)
    want.setflags(write=False)
    scale.setflags(write=False)
    return want, scale


def discrete_variables(name, limit=2):
    _, family = circuit(name)
    found = [v for v, f in enumerate(family) if f in ('Bernoulli', 'Categorical')]
    return found[:1] + found[-1:] if len(found) > limit else found


@functools.lru_cache(maxsize=None)
def oracle_posterior(name, var):
    """(values [V] float32, want [ROWS, V] float64)."""
    d, family = circuit(name)
    ora = oracle(name)
    if family[var] == 'Bernoulli':
        values = np.array([0.0, 1.0], np.float32)
    else:
        values = np.array(sorted({int(c) for L in ora.var_leaves[var] for c in ora.nodes[L]['params']['categories']}),
                          np.float32)
    want = ora.posterior(inputs(name), var, values)
    want.setflags(write=False)
    return values, want
