# DEMCHIPBridge.jl -- included by DEMCHIP.jl (inside `module DEMCHIP`): the binding of include/demc_bridge.h, the header that declares
# the marginal likelihood by bridge sampling on the device.  Same status as DEMCHIP.jl: written against the header, checked against it
# statically (tests/test_bridge_host.py), not executed here.

"the names of demc_bridge's outputs, in the order of out"
const BRIDGE_OUT = (:logml, :re2_prop, :re2_post_iid, :n_iter, :converged, :n_fit, :n1, :n2, :l_star, :n_zero_prop, :n_nonfinite, :rel_change)

"""
    bridge(model::DEModel, de::DE, backend::HIPBackend, n_iter; model_spec::ModelSpec, n_prop=0, seed=0)

The run of `sample`, followed by the log marginal likelihood formed on the device by bridge sampling (demc_bridge, DESIGN.md 5.10) over
rows `offset+1 : offset+Ns` of `bundle_samples` (src/main.jl:222-231, offset = burnin or 0), chains pooled: the first half of the rows
fits a Normal proposal on the real line, the second half and `n_prop` proposal draws (0: as many) feed Meng and Wong's iteration.
Returns a NamedTuple over `BRIDGE_OUT`.  Every model with an exact log posterior is served, the hierarchical, ODE and user-source models
among them; a simulation likelihood is refused with DEMC_EUNSUPPORTED.
"""
function bridge(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::ModelSpec, n_prop::Int = 0, seed::Integer = 0, kwargs...)
    groups = sample_init(model, de, n_iter)
    particles = vcat(groups...)
    P = length(particles); D = length(flatten(particles[1].Θ))
    cfg = make_config(de, D, n_iter, b)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall LIB.demc_create(Ref(cfg)::Ptr{DemcConfig}, href::Ptr{Ptr{Cvoid}})::Int32
    h = href[]
    out = Vector{Float64}(undef, 12)                                     # DEMC_BRIDGE_NOUT
    none = Ptr{Float64}(C_NULL)
    try
        check(h, rc)
        note(h)
        load_handle!(h, model_spec, de, particles)
        run_segments(de, n_iter, [h]) do first, count
            check(h, @ccall LIB.demc_step(h::Ptr{Cvoid}, Int64(first + de.n_initial)::Int64, Int32(count)::Int32)::Int32)
        end
        de.iter = n_iter + de.n_initial
        Ns = de.discard_burnin ? n_iter - de.burnin : n_iter
        offset = de.discard_burnin ? de.burnin : 0
        check(h, @ccall LIB.demc_bridge(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, Int64(n_prop)::Int64, UInt64(seed)::UInt64,
            out::Ptr{Float64}, none::Ptr{Float64}, none::Ptr{Float64}, none::Ptr{Float64})::Int32)
    finally
        h != C_NULL && @ccall LIB.demc_destroy(h::Ptr{Cvoid})::Int32
    end
    return NamedTuple{BRIDGE_OUT}(Tuple(out))
end

"the approximate standard error of logml: sqrt(re2_prop + rho re2_post_iid), rho the autocorrelation factor of the posterior draws"
bridge_se(b::NamedTuple, rho::Real = 1.0) = sqrt(b.re2_prop + rho * b.re2_post_iid)

"""
    compare_bridge(a, b; prior_odds=1.0) -> (log_bf, se, prob_a, prob_b)

Two results of `bridge` for two models of the same data: the log Bayes factor `a.logml - b.logml`, its standard error, and the posterior
model probabilities under `prior_odds = p(a) / p(b)`.
"""
function compare_bridge(a::NamedTuple, b::NamedTuple; prior_odds::Real = 1.0)
    log_bf = a.logml - b.logml
    pa = 1 / (1 + exp(-(log_bf + log(prior_odds))))
    return (log_bf = log_bf, se = sqrt(bridge_se(a)^2 + bridge_se(b)^2), prob_a = pa, prob_b = 1 - pa)
end
