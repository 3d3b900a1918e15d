# GraphicalModelLearningHIP.jl -- the reference-side binding of libgml_hip (include/gml.h).
#
# Drop this file next to the reference package (or `include` it after `using
# GraphicalModelLearning`) and point ENV["LIBGML_HIP"] at libgml_hip.so.  It adds ONE new
# GMLMethod subtype, `HIP`, and the `learn(samples, formulation, ::HIP)` methods; every type,
# constructor and default of GraphicalModelLearning.jl:20-65 is reused unchanged, so
#
#     learn(samples, RISE(), HIP())          # instead of learn(samples, RISE(), NLP())
#
# is the whole migration.  The file only marshals arguments: all arithmetic is in the library.
# NOTE: there is no Julia in the build/test image of this repository, so this file is kept 1:1
# with the Python ctypes binding (graphicalmodellearning.jl_amd/_lib.py), which IS exercised by
# the test-suite on MI355X.
module GraphicalModelLearningHIP

using GraphicalModelLearning
import GraphicalModelLearning: learn, GMLMethod, GMLFormulation, RISE, RISEA, logRISE, RPLE, multiRISE, FactorGraph

export HIP, trim_cache, log_partition

const libgml = get(ENV, "LIBGML_HIP", "libgml_hip.so")

# gml.h constants
const GML_ABI_VERSION = Cint(6)     # the revision of include/gml.h this file mirrors; checked against the library in __init__
const GML_OK, GML_ENOTCONV = Cint(0), Cint(2)
const GML_RISE, GML_LOGRISE, GML_RPLE = Cint(0), Cint(1), Cint(2)
const GML_I64, GML_F64 = Cint(2), Cint(3)
const GML_PREC_F64, GML_PREC_I8X, GML_PREC_AUTO, GML_PREC_I8W = Cint(0), Cint(1), Cint(2), Cint(3)

struct GmlOpts                      # struct gml_opts
    tol::Cdouble; max_iter::Int32; precision::Int32; max_working::Int32; max_add::Int32
    verbose::Int32; hess_samples::Int32; polish::Int32; max_cg::Int32
    limbs_fwd::Int32; hv_limbs_fwd::Int32; hv_limbs_bwd::Int32; debug_row::Int32   # 0 = the library's defaults
    hv_subsample::Int32; coarse::Int32
    cg_viol_frac::Cdouble; cg_eta::Cdouble
end

struct GmlStats                     # struct gml_stats
    iterations::Int32; passes::Int32; forward_passes::Int32; hessian_passes::Int32
    node_evals::Int64; max_kkt::Cdouble; lambda::Cdouble
    t_pack::Cdouble; t_pass::Cdouble; t_hess::Cdouble; t_host::Cdouble; t_total::Cdouble
    not_converged::Int32; polished::Int32
    hv_evals::Int64
    t_assemble::Cdouble
end

# A library built from another revision of gml.h would read GmlOpts / write GmlStats at the wrong offsets without any error:
# refuse it when the module loads (gml.h, "ABI identity").
function __init__()
    v = try
        ccall((:gml_abi_version, libgml), Cint, ())
    catch
        error("$libgml predates gml_abi_version(): rebuild it (this binding is ABI $GML_ABI_VERSION)")
    end
    so, ss = ccall((:gml_sizeof_opts, libgml), Int64, ()), ccall((:gml_sizeof_stats, libgml), Int64, ())
    (v, so, ss) == (GML_ABI_VERSION, sizeof(GmlOpts), sizeof(GmlStats)) ||
        error("$libgml has ABI version / sizeof(gml_opts) / sizeof(gml_stats) = $((v, so, ss)), this binding was written against " *
              "$((GML_ABI_VERSION, sizeof(GmlOpts), sizeof(GmlStats))): library and binding come from different revisions")
end

"""
    HIP(; tol=1e-9, precision=:auto, device=0, devices=nothing, max_iter=100, max_working=512, max_add=64,
        hess_samples=0, polish=true, verbose=0, node_range=nothing)

GMLMethod that solves every node-wise problem on MI355X through libgml_hip (same fields and defaults as the Python
twin, graphicalmodellearning.jl_amd/formulations.py).
`precision = :auto` (default) is `:i8x`, and `:i8w` for tolerances below 2e-10 and for small problems (the reference's fixtures); `:i8x` is the int8-limb fixed-point pass; rows it cannot bring below `tol` are finished on the
FP64 path unless `polish = false`; `:i8w` is the same int8 matrix-core pass at the width of Float64 (theta in 54-bit, the weights in
47-bit limbs, exp in FP64: objective and gradient to the 1e-12 the FP64 path is held to, about 1.5x the time of `:i8x`); `:f64` runs
FP64 MFMA throughout.  `devices = 0:7` shards the nodes over several
GPUs of this node from this one process (gml_multi_*: one handle and one host thread per GPU inside the library, the
row blocks are written straight into the result matrix).
"""
mutable struct HIP <: GMLMethod
    tol::Float64
    precision::Symbol
    device::Int
    devices::Union{Nothing,Vector{Int}}
    max_iter::Int
    max_working::Int
    max_add::Int
    hess_samples::Int
    polish::Bool
    verbose::Int
    node_range::Union{Nothing,Tuple{Int,Int}}   # 1-based inclusive, for one-process-per-GPU sharding
end
HIP(; tol=1e-9, precision=:auto, device=0, devices=nothing, max_iter=100, max_working=512, max_add=64, hess_samples=0,
    polish=true, verbose=0, node_range=nothing) =
    HIP(tol, precision, device, devices === nothing ? nothing : collect(Int, devices), max_iter, max_working, max_add,
        hess_samples, polish, verbose, node_range)

function precision_id(s::Symbol)
    s == :auto && return GML_PREC_AUTO
    s == :i8x && return GML_PREC_I8X
    s == :i8w && return GML_PREC_I8W
    s == :f64 && return GML_PREC_F64
    throw(ArgumentError("HIP: unknown precision :$s (use :auto, :i8x, :i8w or :f64)"))   # as the C ABI and the Python twin do
end

gmlopts(m::HIP) = Ref(GmlOpts(m.tol, m.max_iter, precision_id(m.precision), m.max_working, m.max_add,
                              m.verbose, m.hess_samples, m.polish ? 0 : -1, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0))

lasterr() = unsafe_string(ccall((:gml_last_error, libgml), Cstring, ()))

formulation_id(::Union{RISE,RISEA,multiRISE}) = GML_RISE
formulation_id(::logRISE) = GML_LOGRISE
formulation_id(::RPLE) = GML_RPLE

# rows node0+1 .. node1 of the reconstruction (un-symmetrised), P columns
function solve_rows(samples::Array{T,2}, formulation, method::HIP, order::Int) where T <: Real
    s = T <: AbstractFloat ? convert(Array{Float64,2}, samples) : convert(Array{Int64,2}, samples)
    dtype = eltype(s) == Float64 ? GML_F64 : GML_I64
    K, n = size(s, 1), size(s, 2) - 1
    method.devices === nothing || method.node_range === nothing ||
        throw(ArgumentError("HIP: devices (all nodes over several GPUs) and node_range (one shard) exclude each other"))
    method.devices === nothing || return solve_rows_multi(s, dtype, formulation, method, order)
    n0, n1 = method.node_range === nothing ? (0, n) : (method.node_range[1] - 1, method.node_range[2])
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gml_problem_create, libgml), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
               s, dtype, K, n, K, 1 #= column-major =#, order, n0, n1, method.device, handle)
    rc == GML_OK || error("gml_problem_create: $(lasterr())")
    try
        P = Ref{Int64}(0)
        ccall((:gml_problem_info, libgml), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}),
              handle[], C_NULL, C_NULL, C_NULL, P, C_NULL, C_NULL)
        R = n1 - n0
        out = Array{Float64}(undef, P[], R)          # C row-major (R x P) == Julia (P x R)
        opts = gmlopts(method)
        stats = Ref{GmlStats}()
        rc = ccall((:gml_learn, libgml), Cint,
                   (Ptr{Cvoid}, Cint, Cdouble, Ref{GmlOpts}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GmlStats}),
                   handle[], formulation_id(formulation), Float64(formulation.regularizer), opts, out, C_NULL, stats)
        # the reference: @assert JuMP.termination_status(model) == JuMP.MOI.LOCALLY_SOLVED  (:180)
        rc == GML_ENOTCONV && throw(AssertionError(lasterr()))
        rc == GML_OK || error("gml_learn: $(lasterr())")
        return permutedims(out), nothing, n0             # R x P
    finally
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
    end
end

# The library keeps the device blocks of destroyed handles for the next problem of the same shape (gml.h: gml_trim_cache);
# this hands them back to the driver and returns the number of bytes released.
trim_cache() = Int(ccall((:gml_trim_cache, libgml), Int64, ()))

"""
    stderr(samples, formulation, rows; method=HIP(), structure=nothing, order=2) -> (se, status)

Standard errors of solved rows (gml_stderr: the sandwich covariance A^-1 B A^-1 / M of every node's M-estimator, include/gml.h).
`rows` is the R x P matrix of un-symmetrised solved rows of the nodes `method.node_range` (all nodes by default), `structure` an
R x P `UInt8` matrix of GML_PARAM_* kinds (0 excluded, 1 free, 2 penalised; `nothing` = the field free, the rest penalised).
`se` is R x P (0 outside a row's support), `status[r]` 0 = ok, 1 = singular support, 2 = more than 512 entries (NaN in both cases).
Conditional on the selected support: meant for refitted rows.  Marshalling only.
Not exported: the name shadows `Base.stderr` inside this module only (which does not use the stream); call it as
`GraphicalModelLearningHIP.stderr(...)`.
"""
function stderr(samples::Array{T,2}, formulation, rows::Array{Float64,2}; method::HIP=HIP(),
                structure::Union{Nothing,Array{UInt8,2}}=nothing, order::Int=2) where T <: Real
    s = T <: AbstractFloat ? convert(Array{Float64,2}, samples) : convert(Array{Int64,2}, samples)
    dtype = eltype(s) == Float64 ? GML_F64 : GML_I64
    K, n = size(s, 1), size(s, 2) - 1
    n0, n1 = method.node_range === nothing ? (0, n) : (method.node_range[1] - 1, method.node_range[2])
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gml_problem_create, libgml), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
               s, dtype, K, n, K, 1 #= column-major =#, order, n0, n1, method.device, handle)
    rc == GML_OK || error("gml_problem_create: $(lasterr())")
    try
        R, P = n1 - n0, size(rows, 2)
        size(rows, 1) == R || throw(ArgumentError("stderr: rows has $(size(rows, 1)) rows, the node range has $R"))
        x = permutedims(rows)                             # Julia (P x R) == C row-major (R x P)
        st = structure === nothing ? nothing : permutedims(structure)
        se = Array{Float64}(undef, P, R)
        status = zeros(Int32, R)
        rc = ccall((:gml_stderr, libgml), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64, Ptr{UInt8}, Int64, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}),
                   handle[], formulation_id(formulation), x, P, st === nothing ? C_NULL : st, P, se, status, C_NULL)
        rc == GML_OK || error("gml_stderr: $(lasterr())")
        return permutedims(se), status
    finally
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
    end
end

"""
    log_partition(terms::Dict, n; chains=4096, steps=1000, sweeps_per_step=1, betas=nothing, seed=0, device=0)
        -> (log_z, stderr, ess, log_weights)

log Z of a model of `n` spins given as `Dict(key tuple (1-based spins) => weight)` by annealed importance sampling on the device
(gml_log_partition_ais, include/gml.h): `chains` chains walked along `betas` (default `range(0, 1; length = steps + 1)`; the first
must be 0) with `sweeps_per_step` sweeps at each.  AIS is unbiased for Z, so log_z is biased low; `stderr` is the delta-method
standard error of the chains' weights and does not see a well that no chain found; `ess` near 1 asks for a longer schedule.
Marshalling only.
"""
function log_partition(terms::Dict, n::Integer; chains::Integer=4096, steps::Integer=1000, sweeps_per_step::Integer=1,
                       betas::Union{Nothing,AbstractVector{<:Real}}=nothing, seed::Integer=0, device::Integer=0)
    stride = max(1, maximum(length, keys(terms); init=1))
    keymat = fill(Int32(-1), stride, length(terms))       # Julia (stride x T) == C row-major (T x stride); 0-based, -1 = unused
    weights = Vector{Float64}(undef, length(terms))
    for (t, (key, w)) in enumerate(terms)
        for (a, v) in enumerate(key)
            keymat[a, t] = Int32(v - 1)
        end
        weights[t] = w
    end
    b = betas === nothing ? collect(range(0.0, 1.0; length=steps + 1)) : convert(Vector{Float64}, betas)
    logw = Vector{Float64}(undef, chains)
    result = zeros(Float64, 3)
    rc = ccall((:gml_log_partition_ais, libgml), Cint,
               (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Int64, Ptr{Cdouble}, Int64, Cint, UInt64, Cint,
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int8}, Ptr{Cdouble}),
               keymat, stride, weights, length(weights), n, chains, b, length(b), sweeps_per_step, seed, device,
               logw, C_NULL, C_NULL, result)
    rc == GML_OK || error("gml_log_partition_ais: $(lasterr())")
    return result[1], result[2], result[3], logw
end

"""
    conditional_means(terms::Dict, samples, hidden; replicas=1, samples_per_chain=1, burn_in=200, thin=10, seed=0, device=0)
        -> means (K x H x replicas)

Conditional means of the spins `hidden` (1-based) given the other spins of every row of the histogram `samples` (K x (1+n)), under the
model `Dict(key tuple (1-based spins) => weight)` (gml_conditional_means, include/gml.h): `replicas` Glauber chains per row, started
from the row, the observed spins held fixed, swept over the hidden spins only.  `means[k, a, r]` is the Rao-Blackwellised mean of the
a-th hidden spin (ascending) in replica r of row k, the average of 2 pup - 1 over the recorded sweeps.  The counts of `samples` play no
part.  Marshalling only.
"""
function conditional_means(terms::Dict, samples::Array{T,2}, hidden::AbstractVector{<:Integer}; replicas::Integer=1,
                           samples_per_chain::Integer=1, burn_in::Integer=200, thin::Integer=10, seed::Integer=0,
                           device::Integer=0) where T <: Real
    s = T <: AbstractFloat ? convert(Array{Float64,2}, samples) : convert(Array{Int64,2}, samples)
    dtype = eltype(s) == Float64 ? GML_F64 : GML_I64
    K, n = size(s, 1), size(s, 2) - 1
    all(i -> 1 <= i <= n, hidden) && !isempty(hidden) && allunique(hidden) ||
        throw(ArgumentError("conditional_means: hidden must name distinct spins in 1:$n"))
    mask = zeros(UInt8, n)
    mask[hidden] .= 1
    stride = max(1, maximum(length, keys(terms); init=1))
    keymat = fill(Int32(-1), stride, length(terms))       # Julia (stride x T) == C row-major (T x stride); 0-based, -1 = unused
    weights = Vector{Float64}(undef, length(terms))
    for (t, (key, w)) in enumerate(terms)
        for (a, v) in enumerate(key)
            keymat[a, t] = Int32(v - 1)
        end
        weights[t] = w
    end
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gml_problem_create, libgml), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
               s, dtype, K, n, K, 1 #= column-major =#, 2, 0, n, device, handle)
    rc == GML_OK || error("gml_problem_create: $(lasterr())")
    try
        H = length(hidden)
        means = Array{Float64}(undef, K, replicas, H)     # C row-major [H][replicas][K] == Julia (K x replicas x H)
        rc = ccall((:gml_conditional_means, libgml), Cint,
                   (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Cvoid}, Ptr{UInt8}, Cint, Int64, Cint, Cint, UInt64, Ptr{Cdouble}),
                   keymat, stride, weights, length(weights), n, handle[], mask, replicas, samples_per_chain, burn_in, thin, seed, means)
        rc == GML_OK || error("gml_conditional_means: $(lasterr())")
        return permutedims(means, (1, 3, 2))
    finally
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
    end
end

# the term list of a Dict(key tuple (1-based spins) => weight) as the C ABI takes it: (keymat (stride x T) Int32, 0-based, -1 = unused;
# weights; stride)
function term_arrays(terms::Dict)
    stride = max(1, maximum(length, keys(terms); init=1))
    keymat = fill(Int32(-1), stride, length(terms))       # Julia (stride x T) == C row-major (T x stride)
    weights = Vector{Float64}(undef, length(terms))
    for (t, (key, w)) in enumerate(terms)
        for (a, v) in enumerate(key)
            keymat[a, t] = Int32(v - 1)
        end
        weights[t] = w
    end
    return keymat, weights, stride
end

"""
    conditional_exact(terms::Dict, samples, hidden; device=0) -> means (K x H), log_w (K), log_p (K)

Exact conditional inference (gml_conditional_exact, include/gml.h): the spins `hidden` (1-based, at most 24) of every row of the
histogram `samples` (K x (1+n)) are enumerated on the device, no chain.  `means[k, a]` = E[s | the visible spins of row k] of the a-th
hidden spin (ascending); `log_w[k]` = log sum over the hidden spins of exp(E), so log P(visible spins of row k) = log_w[k] - log Z;
`log_p[k]` = log P(the values row k holds on the hidden spins | its visible spins).  The counts of `samples` play no part.
Marshalling only.
"""
function conditional_exact(terms::Dict, samples::Array{T,2}, hidden::AbstractVector{<:Integer}; device::Integer=0) where T <: Real
    s = T <: AbstractFloat ? convert(Array{Float64,2}, samples) : convert(Array{Int64,2}, samples)
    dtype = eltype(s) == Float64 ? GML_F64 : GML_I64
    K, n = size(s, 1), size(s, 2) - 1
    all(i -> 1 <= i <= n, hidden) && !isempty(hidden) && allunique(hidden) ||
        throw(ArgumentError("conditional_exact: hidden must name distinct spins in 1:$n"))
    mask = zeros(UInt8, n)
    mask[hidden] .= 1
    keymat, weights, stride = term_arrays(terms)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gml_problem_create, libgml), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
               s, dtype, K, n, K, 1 #= column-major =#, 2, 0, n, device, handle)
    rc == GML_OK || error("gml_problem_create: $(lasterr())")
    try
        means = Array{Float64}(undef, K, length(hidden))  # C row-major [H][K] == Julia (K x H)
        log_w = Vector{Float64}(undef, K)
        log_p = Vector{Float64}(undef, K)
        rc = ccall((:gml_conditional_exact, libgml), Cint,
                   (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                   keymat, stride, weights, length(weights), n, handle[], mask, means, log_w, log_p)
        rc == GML_OK || error("gml_conditional_exact: $(lasterr())")
        return means, log_w, log_p
    finally
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
    end
end

"""
    conditional_exact_masked(terms::Dict, samples; device=0) -> means (K x n), log_w (K), log_p (K)

The same for data with holes (gml_conditional_exact_masked): a spin entry of `samples` (K x (1+n)) is -1, +1 or 0 = missing, at most 24
missing per row, and every row's own missing spins are enumerated.  `means[k, i]` is the exact conditional mean where row k lacks spin
i and the observed value where it does not; `log_w[k]` - log Z is the marginal log-likelihood of what row k observes.  Two handles
are made and destroyed: the evidence (a hole holds +1, which plays no part) and the mask (-1 = missing).  Marshalling only.
"""
function conditional_exact_masked(terms::Dict, samples::Array{T,2}; device::Integer=0) where T <: Real
    K, n = size(samples, 1), size(samples, 2) - 1
    spins = samples[:, 2:end]
    all(v -> v == -1 || v == 0 || v == 1, spins) || throw(ArgumentError("conditional_exact_masked: spin entries must be -1, +1 or 0"))
    evidence = Int8.(ifelse.(spins .== 0, 1, spins))
    holes = Int8.(ifelse.(spins .== 0, -1, 1))
    keymat, weights, stride = term_arrays(terms)
    he = Ref{Ptr{Cvoid}}(C_NULL)
    hm = Ref{Ptr{Cvoid}}(C_NULL)
    create(bytes, h) = ccall((:gml_problem_create_spins, libgml), Cint,
                             (Ptr{Cdouble}, Ptr{Int8}, Int64, Int64, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
                             C_NULL, bytes, K, n, 2, 0, n, device, h)
    rc = create(permutedims(evidence), he)                # (C row-major [K][n] bytes == Julia (n x K); counts NULL: all ones)
    rc == GML_OK || error("gml_problem_create_spins: $(lasterr())")
    try
        rc = create(permutedims(holes), hm)
        rc == GML_OK || error("gml_problem_create_spins: $(lasterr())")
        means = Array{Float64}(undef, K, n)               # C row-major [n][K] == Julia (K x n)
        log_w = Vector{Float64}(undef, K)
        log_p = Vector{Float64}(undef, K)
        rc = ccall((:gml_conditional_exact_masked, libgml), Cint,
                   (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                   keymat, stride, weights, length(weights), n, he[], hm[], means, log_w, log_p)
        rc == GML_OK || error("gml_conditional_exact_masked: $(lasterr())")
        return means, log_w, log_p
    finally
        hm[] == C_NULL || ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), hm[])
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), he[])
    end
end

"""
    most_probable_states(terms::Dict, n, k=1; device=0) -> states (found x n, Int8 +-1), energies (found)

The found = min(k, 2^n) most probable states of a model of `n` spins (gml_model_best_states, include/gml.h), certified by enumeration
on the device: energy descending, equal energies in state order (spin i at bit i - 1, -1 a set bit, the smaller number first).
1 <= k <= 256, connected components of at most 40 spins.  Marshalling only.
"""
function most_probable_states(terms::Dict, n::Integer, k::Integer=1; device::Integer=0)
    keymat, weights, stride = term_arrays(terms)
    rows = clamp(k, 0, 256)                                # (the library refuses a k outside 1:256 before it writes)
    states = Array{Int8}(undef, n, rows)                   # C row-major [k][n] == Julia (n x k)
    energies = Vector{Float64}(undef, rows)
    found = Ref{Int64}(0)
    rc = ccall((:gml_model_best_states, libgml), Cint,
               (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Int64, Cint, Ref{Int64}, Ptr{Int8}, Ptr{Cdouble}),
               keymat, stride, weights, length(weights), n, k, device, found, states, energies)
    rc == GML_OK || error("gml_model_best_states: $(lasterr())")
    return permutedims(states[:, 1:found[]]), energies[1:found[]]
end

"""
    conditional_mode(terms::Dict, samples, hidden; device=0) -> states (K x H, Int8 +-1), energy (K), log_p (K)

The most probable joint state of the spins `hidden` (1-based, at most 24) given the other spins of every row of the histogram
`samples` (K x (1+n)) (gml_conditional_mode, include/gml.h): `states[k, a]` is the value of the a-th hidden spin (ascending),
`energy[k]` the row's energy at that state, `log_p[k]` its conditional log-probability.  Marshalling only.
"""
function conditional_mode(terms::Dict, samples::Array{T,2}, hidden::AbstractVector{<:Integer}; device::Integer=0) where T <: Real
    s = T <: AbstractFloat ? convert(Array{Float64,2}, samples) : convert(Array{Int64,2}, samples)
    dtype = eltype(s) == Float64 ? GML_F64 : GML_I64
    K, n = size(s, 1), size(s, 2) - 1
    all(i -> 1 <= i <= n, hidden) && !isempty(hidden) && allunique(hidden) ||
        throw(ArgumentError("conditional_mode: hidden must name distinct spins in 1:$n"))
    mask = zeros(UInt8, n)
    mask[hidden] .= 1
    keymat, weights, stride = term_arrays(terms)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gml_problem_create, libgml), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
               s, dtype, K, n, K, 1 #= column-major =#, 2, 0, n, device, handle)
    rc == GML_OK || error("gml_problem_create: $(lasterr())")
    try
        states = Array{Int8}(undef, K, length(hidden))    # C row-major [H][K] == Julia (K x H)
        energy = Vector{Float64}(undef, K)
        log_p = Vector{Float64}(undef, K)
        rc = ccall((:gml_conditional_mode, libgml), Cint,
                   (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int8}, Ptr{Cdouble}, Ptr{Cdouble}),
                   keymat, stride, weights, length(weights), n, handle[], mask, states, energy, log_p)
        rc == GML_OK || error("gml_conditional_mode: $(lasterr())")
        return states, energy, log_p
    finally
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
    end
end

"""
    conditional_mode_masked(terms::Dict, samples; device=0) -> completed (K x n, Int8 +-1), energy (K), log_p (K)

The same for data with holes (gml_conditional_mode_masked): a spin entry of `samples` (K x (1+n)) is -1, +1 or 0 = missing, at most 24
missing per row; `completed[k, :]` is row k with its missing entries filled by their most probable joint values, the observed ones
kept.  Two handles are made and destroyed, as in conditional_exact_masked.  Marshalling only.
"""
function conditional_mode_masked(terms::Dict, samples::Array{T,2}; device::Integer=0) where T <: Real
    K, n = size(samples, 1), size(samples, 2) - 1
    spins = samples[:, 2:end]
    all(v -> v == -1 || v == 0 || v == 1, spins) || throw(ArgumentError("conditional_mode_masked: spin entries must be -1, +1 or 0"))
    evidence = Int8.(ifelse.(spins .== 0, 1, spins))
    holes = Int8.(ifelse.(spins .== 0, -1, 1))
    keymat, weights, stride = term_arrays(terms)
    he = Ref{Ptr{Cvoid}}(C_NULL)
    hm = Ref{Ptr{Cvoid}}(C_NULL)
    create(bytes, h) = ccall((:gml_problem_create_spins, libgml), Cint,
                             (Ptr{Cdouble}, Ptr{Int8}, Int64, Int64, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
                             C_NULL, bytes, K, n, 2, 0, n, device, h)
    rc = create(permutedims(evidence), he)
    rc == GML_OK || error("gml_problem_create_spins: $(lasterr())")
    try
        rc = create(permutedims(holes), hm)
        rc == GML_OK || error("gml_problem_create_spins: $(lasterr())")
        completed = Array{Int8}(undef, K, n)              # C row-major [n][K] == Julia (K x n)
        energy = Vector{Float64}(undef, K)
        log_p = Vector{Float64}(undef, K)
        rc = ccall((:gml_conditional_mode_masked, libgml), Cint,
                   (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int8}, Ptr{Cdouble}, Ptr{Cdouble}),
                   keymat, stride, weights, length(weights), n, he[], hm[], completed, energy, log_p)
        rc == GML_OK || error("gml_conditional_mode_masked: $(lasterr())")
        return completed, energy, log_p
    finally
        hm[] == C_NULL || ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), hm[])
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), he[])
    end
end

"""
    conditional_draw(terms::Dict, samples, hidden; replicas=1, seed=0, device=0)
        -> states (K*replicas x H, Int8 +-1), energy (K*replicas), log_p (K*replicas)

Exact draws of the spins `hidden` (1-based, at most 24) given the other spins of every row of the histogram `samples` (K x (1+n))
(gml_conditional_draw, include/gml.h; Gumbel-max over the row's enumeration, no chain): row `r*K + k` (0-based) of the results is
replica r of row k -- `states[c, a]` the value of the a-th hidden spin (ascending), `energy[c]` the unperturbed energy of the draw,
`log_p[c]` its conditional log-probability.  Marshalling only.
"""
function conditional_draw(terms::Dict, samples::Array{T,2}, hidden::AbstractVector{<:Integer}; replicas::Integer=1, seed::Integer=0,
                          device::Integer=0) where T <: Real
    s = T <: AbstractFloat ? convert(Array{Float64,2}, samples) : convert(Array{Int64,2}, samples)
    dtype = eltype(s) == Float64 ? GML_F64 : GML_I64
    K, n = size(s, 1), size(s, 2) - 1
    all(i -> 1 <= i <= n, hidden) && !isempty(hidden) && allunique(hidden) ||
        throw(ArgumentError("conditional_draw: hidden must name distinct spins in 1:$n"))
    replicas >= 1 || throw(ArgumentError("conditional_draw: replicas must be at least 1"))
    mask = zeros(UInt8, n)
    mask[hidden] .= 1
    keymat, weights, stride = term_arrays(terms)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gml_problem_create, libgml), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
               s, dtype, K, n, K, 1 #= column-major =#, 2, 0, n, device, handle)
    rc == GML_OK || error("gml_problem_create: $(lasterr())")
    try
        chains = K * replicas
        states = Array{Int8}(undef, chains, length(hidden))    # C row-major [H][K replicas] == Julia (K replicas x H)
        energy = Vector{Float64}(undef, chains)
        log_p = Vector{Float64}(undef, chains)
        rc = ccall((:gml_conditional_draw, libgml), Cint,
                   (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Cvoid}, Ptr{UInt8}, Cint, UInt64, Ptr{Int8}, Ptr{Cdouble},
                    Ptr{Cdouble}),
                   keymat, stride, weights, length(weights), n, handle[], mask, replicas, seed, states, energy, log_p)
        rc == GML_OK || error("gml_conditional_draw: $(lasterr())")
        return states, energy, log_p
    finally
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
    end
end

"""
    conditional_draw_masked(terms::Dict, samples; replicas=1, seed=0, device=0)
        -> completed (K*replicas x n, Int8 +-1), energy (K*replicas), log_p (K*replicas)

The same for data with holes (gml_conditional_draw_masked): a spin entry of `samples` (K x (1+n)) is -1, +1 or 0 = missing, at most 24
missing per row; `completed[r*K + k, :]` (0-based) is row k with its missing entries drawn from their joint conditional distribution,
the observed ones kept.  Two handles are made and destroyed, as in conditional_mode_masked.  Marshalling only.
"""
function conditional_draw_masked(terms::Dict, samples::Array{T,2}; replicas::Integer=1, seed::Integer=0,
                                 device::Integer=0) where T <: Real
    K, n = size(samples, 1), size(samples, 2) - 1
    spins = samples[:, 2:end]
    all(v -> v == -1 || v == 0 || v == 1, spins) || throw(ArgumentError("conditional_draw_masked: spin entries must be -1, +1 or 0"))
    replicas >= 1 || throw(ArgumentError("conditional_draw_masked: replicas must be at least 1"))
    evidence = Int8.(ifelse.(spins .== 0, 1, spins))
    holes = Int8.(ifelse.(spins .== 0, -1, 1))
    keymat, weights, stride = term_arrays(terms)
    he = Ref{Ptr{Cvoid}}(C_NULL)
    hm = Ref{Ptr{Cvoid}}(C_NULL)
    create(bytes, h) = ccall((:gml_problem_create_spins, libgml), Cint,
                             (Ptr{Cdouble}, Ptr{Int8}, Int64, Int64, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
                             C_NULL, bytes, K, n, 2, 0, n, device, h)
    rc = create(permutedims(evidence), he)
    rc == GML_OK || error("gml_problem_create_spins: $(lasterr())")
    try
        rc = create(permutedims(holes), hm)
        rc == GML_OK || error("gml_problem_create_spins: $(lasterr())")
        chains = K * replicas
        completed = Array{Int8}(undef, chains, n)         # C row-major [n][K replicas] == Julia (K replicas x n)
        energy = Vector{Float64}(undef, chains)
        log_p = Vector{Float64}(undef, chains)
        rc = ccall((:gml_conditional_draw_masked, libgml), Cint,
                   (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cint, UInt64, Ptr{Int8}, Ptr{Cdouble},
                    Ptr{Cdouble}),
                   keymat, stride, weights, length(weights), n, he[], hm[], replicas, seed, completed, energy, log_p)
        rc == GML_OK || error("gml_conditional_draw_masked: $(lasterr())")
        return completed, energy, log_p
    finally
        hm[] == C_NULL || ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), hm[])
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), he[])
    end
end

# a caller's elimination order (1-based spins) as the C ABI takes it, or C_NULL for the library's greedy order
elim_order(order, n) = order === nothing ? Ptr{Int32}(C_NULL) :
    (length(order) == n || throw(ArgumentError("order must name each of the $n spins once")); Int32.(order .- 1))

"""
    model_elim_plan(terms::Dict, n; order=nothing) -> order (n, 1-based), width, work, stored

The elimination order of a model of `n` spins and what it costs (gml_model_elim_plan, include/gml.h): the largest scope of a step,
sum_t 2^|scope_t| and sum_t 2^|F_t|.  `order`: a permutation of 1:n, or `nothing` for the greedy order.  Host only; marshalling only.
"""
function model_elim_plan(terms::Dict, n::Integer; order=nothing)
    keymat, weights, stride = term_arrays(terms)
    out = Vector{Int32}(undef, n)
    width, work, stored = Ref{Int32}(0), Ref{Cdouble}(0), Ref{Cdouble}(0)
    rc = ccall((:gml_model_elim_plan, libgml), Cint,
               (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Int32}, Ptr{Int32}, Ref{Int32}, Ref{Cdouble}, Ref{Cdouble}),
               keymat, stride, weights, length(weights), n, elim_order(order, n), out, width, work, stored)
    rc == GML_OK || error("gml_model_elim_plan: $(lasterr())")
    return Int.(out) .+ 1, Int(width[]), work[], stored[]
end

"""
    model_elim(terms::Dict, n; order=nothing, device=0) -> log_z, mean (n), texp (length(terms), in the Dict's iteration order)

Exact log Z, means and the expectation of every term of a sparse model of `n` spins by variable elimination on the device
(gml_model_elim, include/gml.h): elimination orders of width at most 30.  Marshalling only.
"""
function model_elim(terms::Dict, n::Integer; order=nothing, device::Integer=0)
    keymat, weights, stride = term_arrays(terms)
    log_z = Ref{Cdouble}(0)
    mean = Vector{Float64}(undef, n)
    texp = Vector{Float64}(undef, length(weights))
    rc = ccall((:gml_model_elim, libgml), Cint,
               (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Int32}, Cint, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               keymat, stride, weights, length(weights), n, elim_order(order, n), device, log_z, mean, texp)
    rc == GML_OK || error("gml_model_elim: $(lasterr())")
    return log_z[], mean, texp
end

"""
    sample_elim(terms::Dict, n, N; seed=0, order=nothing, device=0) -> counts (K), spins (K x n, +-1)

`N` exact, independent draws of a sparse model of `n` spins by backward sampling on the tables of variable elimination
(gml_problem_create_sampled_elim, include/gml.h): elimination orders of width at most 30, no chain and no burn-in.  For n <= 64 and
N < 2^31 the distinct configurations with their counts (histogrammed on the device), otherwise one row of count 1 per draw.
Marshalling only.
"""
function sample_elim(terms::Dict, n::Integer, N::Integer; seed::Integer=0, order=nothing, device::Integer=0)
    keymat, weights, stride = term_arrays(terms)
    porder = max(2, maximum(length, keys(terms)))
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gml_problem_create_sampled_elim, libgml), Cint,
               (Ptr{Int32}, Cint, Ptr{Cdouble}, Int64, Int64, Int64, UInt64, Ptr{Int32}, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
               keymat, stride, weights, length(weights), n, N, seed, elim_order(order, n), (n <= 64 && N < 2^31) ? 1 : 0, porder, 0, n,
               device, handle)
    rc == GML_OK || error("gml_problem_create_sampled_elim: $(lasterr())")
    try
        K = Ref{Int64}(0)
        ccall((:gml_problem_info, libgml), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}, Ptr{Cdouble}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
              handle[], C_NULL, K, C_NULL, C_NULL, C_NULL, C_NULL)
        rows = Matrix{Int8}(undef, n, K[])  # (the library writes row-major [K][n])
        counts = Vector{Float64}(undef, K[])
        rc = ccall((:gml_problem_get_spins, libgml), Cint, (Ptr{Cvoid}, Ptr{Int8}), handle[], rows)
        rc == GML_OK || error("gml_problem_get_spins: $(lasterr())")
        rc = ccall((:gml_problem_get_counts, libgml), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), handle[], counts)
        rc == GML_OK || error("gml_problem_get_counts: $(lasterr())")
        return counts, permutedims(rows)
    finally
        ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
    end
end

# all nodes over method.devices: gml_multi_* (one handle + one host thread per GPU inside the library)
function solve_rows_multi(s, dtype, formulation, method::HIP, order::Int)
    K, n = size(s, 1), size(s, 2) - 1
    devs = convert(Vector{Cint}, method.devices)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gml_multi_create, libgml), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Ptr{Cint}, Cint, Ref{Ptr{Cvoid}}),
               s, dtype, K, n, K, 1, order, devs, length(devs), handle)
    rc == GML_OK || error("gml_multi_create: $(lasterr())")
    try
        P = Ref{Int64}(0)
        ccall((:gml_multi_info, libgml), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ptr{Cint}, Ptr{UInt8}),
              handle[], C_NULL, C_NULL, C_NULL, P, C_NULL, C_NULL)
        out = Array{Float64}(undef, P[], n)               # C row-major (n x P) == Julia (P x n)
        stats = Ref{GmlStats}()
        rc = ccall((:gml_multi_learn, libgml), Cint,
                   (Ptr{Cvoid}, Cint, Cdouble, Ref{GmlOpts}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GmlStats}, Ptr{Ptr{Cdouble}}),
                   handle[], formulation_id(formulation), Float64(formulation.regularizer), gmlopts(method), out, C_NULL, stats, C_NULL)
        rc == GML_ENOTCONV && throw(AssertionError(lasterr()))   # @assert ... LOCALLY_SOLVED (:180)
        rc == GML_OK || error("gml_multi_learn: $(lasterr())")
        return permutedims(out), nothing, 0
    finally
        ccall((:gml_multi_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
    end
end

# RISE / logRISE / RPLE / RISEA: n x n matrix, diagonal = fields  (:154-189, :263-298, :301-336, :210-260)
# One GPU, all nodes: gml_learn_matrix -- the solve and `0.5 * (reconstruction + transpose(reconstruction))` (:184-186) in one call,
# the rows never leaving the device (on the host that line walks the transposed operand with a stride of n doubles: 0.2 s at n = 4096).
# Node shards and several GPUs: the gathered rows through gml_matrix_symmetrize.
function learn(samples::Array{T,2}, formulation::Union{RISE,RISEA,logRISE,RPLE}, method::HIP) where T <: Real
    n = size(samples, 2) - 1
    if method.devices === nothing && method.node_range === nothing && formulation.symmetrization
        s = T <: AbstractFloat ? convert(Array{Float64,2}, samples) : convert(Array{Int64,2}, samples)
        K = size(s, 1)
        handle = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:gml_problem_create, libgml), Cint,
                   (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
                   s, eltype(s) == Float64 ? GML_F64 : GML_I64, K, n, K, 1, 2, 0, n, method.device, handle)
        rc == GML_OK || error("gml_problem_create: $(lasterr())")
        try
            out = Array{Float64}(undef, n, n)             # symmetric: row-major and column-major coincide
            stats = Ref{GmlStats}()
            rc = ccall((:gml_learn_matrix, libgml), Cint,
                       (Ptr{Cvoid}, Cint, Cdouble, Cint, Ref{GmlOpts}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GmlStats}),
                       handle[], formulation_id(formulation), Float64(formulation.regularizer), Cint(1), gmlopts(method), out, C_NULL, stats)
            rc == GML_ENOTCONV && throw(AssertionError(lasterr()))              # @assert ... LOCALLY_SOLVED (:180)
            rc == GML_OK || error("gml_learn_matrix: $(lasterr())")
            return out
        finally
            ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
        end
    end
    reconstruction, _, _ = solve_rows(samples, formulation, method, 2)
    if formulation.symmetrization && size(reconstruction, 1) == size(reconstruction, 2)
        rt = permutedims(reconstruction)                                          # C row-major n x n
        rc = ccall((:gml_matrix_symmetrize, libgml), Cint, (Ptr{Cdouble}, Int64, Int64, Cint, Ptr{Cdouble}),
                   rt, n, n, method.devices === nothing ? method.device : method.devices[1], rt)   # :184-186, in place
        rc == GML_OK || error("gml_matrix_symmetrize: $(lasterr())")
        reconstruction = rt                                                       # symmetric: no transpose back needed
    end
    return reconstruction
end

# multiRISE: FactorGraph keyed by (u, ascending others), optionally symmetrised  (:83-152).
# The per-key storage (:129-132), the grouping by sorted key and the `mean` (:135-149) run on the device (gml_learn_terms /
# gml_terms_assemble: one kernel, keys <-> positions in closed form); what comes back is ONE weight vector in the order the
# reference lists a model's terms in (models.jl:61,72: by (length, key)) and the matching key table from gml_terms_keys, and the
# Dict the FactorGraph constructor wants is built from the two in a single comprehension.
function learn(samples::Array{T,2}, formulation::multiRISE, method::HIP) where T <: Real
    order = formulation.interaction_order
    n = size(samples, 2) - 1
    sym = formulation.symmetrization ? Cint(1) : Cint(0)
    nterms = ccall((:gml_terms_count, libgml), Int64, (Int64, Cint, Cint), n, order, sym)
    nterms >= 0 || error("gml_terms_count: $(lasterr())")
    weights = Vector{Float64}(undef, nterms)
    if method.devices === nothing && method.node_range === nothing
        # one GPU, all nodes: solve + assembly in one call, the n x P rows never leave the device
        s = T <: AbstractFloat ? convert(Array{Float64,2}, samples) : convert(Array{Int64,2}, samples)
        K = size(s, 1)
        handle = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:gml_problem_create, libgml), Cint,
                   (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
                   s, eltype(s) == Float64 ? GML_F64 : GML_I64, K, n, K, 1, order, 0, n, method.device, handle)
        rc == GML_OK || error("gml_problem_create: $(lasterr())")
        try
            stats = Ref{GmlStats}()
            rc = ccall((:gml_learn_terms, libgml), Cint,
                       (Ptr{Cvoid}, Cint, Cdouble, Cint, Ref{GmlOpts}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GmlStats}),
                       handle[], GML_RISE, Float64(formulation.regularizer), sym, gmlopts(method), weights, C_NULL, stats)
            rc == GML_ENOTCONV && throw(AssertionError(lasterr()))                # @assert ... LOCALLY_SOLVED (:127)
            rc == GML_OK || error("gml_learn_terms: $(lasterr())")
        finally
            ccall((:gml_problem_destroy, libgml), Cvoid, (Ptr{Cvoid},), handle[])
        end
    else
        method.node_range === nothing ||
            throw(ArgumentError("HIP: multiRISE assembles a FactorGraph from the rows of all nodes; node_range solves a shard"))
        rows, _, _ = solve_rows(samples, formulation, method, order)              # n x P (gml_multi_learn over method.devices)
        rt = permutedims(rows)                                                    # back to C row-major n x P
        rc = ccall((:gml_terms_assemble, libgml), Cint, (Ptr{Cdouble}, Int64, Int64, Cint, Cint, Cint, Ptr{Cdouble}),
                   rt, size(rt, 1), n, order, sym, method.devices[1], weights)
        rc == GML_OK || error("gml_terms_assemble: $(lasterr())")
    end
    keys = Array{Int32}(undef, order, nterms)                                     # C [nterms][order], 0-based, -1 = unused slot
    rc = ccall((:gml_terms_keys, libgml), Cint, (Int64, Cint, Cint, Int64, Int64, Ptr{Int32}), n, order, sym, 0, nterms, keys)
    rc == GML_OK || error("gml_terms_keys: $(lasterr())")
    reconstruction = Dict{Tuple,Real}(tuple((Int(k) + 1 for k in view(keys, :, t) if k >= 0)...) => weights[t] for t in 1:nterms)
    return FactorGraph(order, n, :spin, reconstruction)                           # :151
end

end # module
