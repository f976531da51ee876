# DEMCHIPSummary.jl -- included by DEMCHIP.jl (inside `module DEMCHIP`): the binding of include/demc_summary.h, the header that
# stands next to include/demc.h and declares the one call that follows a run.  Same status as DEMCHIP.jl: written against the
# header, checked against it statically (tests/test_summary_host.py), not executed here.

"""
    summarize(model::DEModel, de::DE, backend::HIPBackend, n_iter; model_spec, max_lag=0)

The run of `sample`, followed by `describe(chains)` computed on the device (demc_summarize, DESIGN.md 5.5) instead of an export of
the history: rows `offset+1 : offset+Ns` of `bundle_samples` (src/main.jl:222-231, offset = burnin or 0).  Returns
`(names, table)` with `table[j, :] = (mean, std, rhat, ess, mcse, pairs)` of series `names[j]` -- the names of `get_names`:
the parameters, then acceptance and lp.  ess is the split-chain form without rank normalisation and without Stan's antithetic tail term:
MCMCChains' `ess_rhat` differs from it by those two steps; `rankstats` (DEMCHIPRank.jl) gives the rank-normalised columns.
"""
function summarize(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::AnyModelSpec, max_lag::Int = 0, kwargs...)
    groups = sample_init(model, de, n_iter)
    particles = vcat(groups...)
    P = length(particles); D = length(flatten(particles[1].Θ))
    cfg = make_config(de, D, n_iter, b)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall LIB.demc_create(Ref(cfg)::Ptr{DemcConfig}, href::Ptr{Ptr{Cvoid}})::Int32
    h = href[]
    out = Matrix{Float64}(undef, 6, D + 2)                               # C order [D+2][6]
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
        check(h, @ccall LIB.demc_summarize(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, Int32(max_lag)::Int32,
            out::Ptr{Float64}, C_NULL::Ptr{Float64}, 0::Int64)::Int32)
    finally
        h != C_NULL && @ccall LIB.demc_destroy(h::Ptr{Cvoid})::Int32
    end
    names = DifferentialEvolutionMCMC.get_names(model, particles[1])            # (utilities.jl:131-149: ends with acceptance, lp)
    return names, permutedims(out)
end
