# DEMCHIPQuantile.jl -- included by DEMCHIP.jl (inside `module DEMCHIP`): the binding of include/demc_quantile.h, the header that
# declares the second table of describe(chains).  Same status as DEMCHIP.jl: written against the header, checked against it
# statically (tests/test_quantile_host.py), not executed here.

const DEFAULT_QUANTILES = [0.025, 0.25, 0.5, 0.75, 0.975]                      # describe(chains)[2]

"""
    quantiles(model::DEModel, de::DE, backend::HIPBackend, n_iter; model_spec, q=DEFAULT_QUANTILES)

The run of `sample`, followed by `quantile(chains; q)` selected on the device (demc_quantiles, DESIGN.md 5.6) instead of an export
of the history: rows `offset+1 : offset+Ns` of `bundle_samples` (src/main.jl:222-231, offset = burnin or 0), chains pooled as
MCMCChains pools them.  Returns `(names, table)` with `table[j, k]` the quantile `q[k]` of series `names[j]` -- the names of
`get_names`: the parameters, then acceptance and lp.  The definition is `Statistics.quantile`'s default (type 7) on the values in
IEEE order, exact to the bit; a series that holds a NaN has NaN throughout.
"""
function quantiles(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::AnyModelSpec, q::Vector{Float64} = DEFAULT_QUANTILES, kwargs...)
    groups = sample_init(model, de, n_iter)
    particles = vcat(groups...)
    P = length(particles); D = length(flatten(particles[1].Θ))
    cfg = make_config(de, D, n_iter, b)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall LIB.demc_create(Ref(cfg)::Ptr{DemcConfig}, href::Ptr{Ptr{Cvoid}})::Int32
    h = href[]
    out = Matrix{Float64}(undef, length(q), D + 2)                       # C order [D+2][n_probs]
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
        check(h, @ccall LIB.demc_quantiles(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, q::Ptr{Float64},
            Int32(length(q))::Int32, out::Ptr{Float64})::Int32)
    finally
        h != C_NULL && @ccall LIB.demc_destroy(h::Ptr{Cvoid})::Int32
    end
    names = DifferentialEvolutionMCMC.get_names(model, particles[1])            # (utilities.jl:131-149: ends with acceptance, lp)
    return names, permutedims(out)
end
