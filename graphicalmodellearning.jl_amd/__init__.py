"""MI355X-native learn() hot path of GraphicalModelLearning.jl.

Same surface as the reference module (GraphicalModelLearning.jl:3-6, models.jl:3): learn,
the GMLFormulation types, the GMLMethod types (NLP plus the new HIP), FactorGraph.  The compute
path is libgml_hip.so (hand-written HIP kernels for gfx950 behind the C ABI in include/gml.h).
"""
from . import inference  # noqa: F401
from ._lib import (EXCLUDED, FREE, PENALISED, GMLConvergenceError, GMLError, MultiProblem, Problem, lib, moments,  # noqa: F401
                   structure_from_keys, structure_from_rows)
from .factor_graph import FactorGraph, matrix_to_terms, permutations, check_model_data  # noqa: F401
from .formulations import (HIP, ISODUS, NLP, RISE, RISEA, RPLE, GMLFormulation, GMLMethod,  # noqa: F401
                           logRISE, multiRISE)
from .inference import (ConditionalMeans, ConditionalMode, Imputation, ImputedMode, PredictiveCheck, conditional_means,  # noqa: F401
                        conditional_mode, conditional_sample, impute, impute_mode, impute_sample, predictive_check)
from .learn import learn  # noqa: F401
from .likelihood import (AIS, Elimination, Exact, LogLikelihood, LogPartition, MostProbable, exact_moments, log_likelihood,  # noqa: F401
                         log_partition, model_term_moments, most_probable_states, observed_log_likelihood)
from .missing import EMStep, ImputationEM, MissingDataResult, learn_missing  # noqa: F401
from .path import PathResult, learn_path  # noqa: F401
from .sampling import GMSampler, Gibbs, Glauber, GlauberChains, GlauberTermChains, TemperedTermChains, sample  # noqa: F401

__all__ = ["learn", "GMLFormulation", "RISE", "logRISE", "RPLE", "RISEA", "multiRISE", "ISODUS", "GMLMethod",
           "NLP", "HIP", "FactorGraph", "Problem", "MultiProblem", "GMLError", "GMLConvergenceError", "sample", "GMSampler", "Gibbs",
           "Glauber", "GlauberChains", "GlauberTermChains", "TemperedTermChains", "moments", "EXCLUDED", "FREE", "PENALISED",
           "structure_from_rows", "structure_from_keys", "learn_path", "PathResult", "AIS", "log_partition", "log_likelihood", "LogPartition",
           "LogLikelihood", "conditional_sample", "conditional_means", "predictive_check", "ConditionalMeans", "PredictiveCheck",
           "impute", "impute_sample", "Imputation", "learn_missing", "ImputationEM", "EMStep", "MissingDataResult", "Exact",
           "exact_moments", "observed_log_likelihood", "most_probable_states", "MostProbable", "conditional_mode", "ConditionalMode",
           "impute_mode", "ImputedMode", "Elimination", "model_term_moments"]
