# DEMCHIPRank.jl -- included by DEMCHIP.jl (inside `module DEMCHIP`): the binding of include/demc_rank.h, the header that declares the
# rank-normalised chain diagnostics on the device.  Same status as DEMCHIP.jl: written against the header, checked against it
# statically (tests/test_rank_host.py), not executed here.

"the columns of demc_rankstats' table, in the order of out"
const RANK_COLS = (:rhat, :ess_bulk, :ess_tail, :rhat_bulk, :rhat_folded, :ess_q05, :ess_q95, :distinct)

function run_then(f, model::DEModel, de::DE, b::HIPBackend, n_iter::Int, model_spec)
    groups = sample_init(model, de, n_iter)
    particles = vcat(groups...)
    P = length(particles); D = length(flatten(particles[1].Θ))
    cfg = make_config(de, D, n_iter, b)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall LIB.demc_create(Ref(cfg)::Ptr{DemcConfig}, href::Ptr{Ptr{Cvoid}})::Int32
    h = href[]
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
        return f(h, particles, P, D, offset, Ns)
    finally
        h != C_NULL && @ccall LIB.demc_destroy(h::Ptr{Cvoid})::Int32
    end
end

"""
    rankstats(model::DEModel, de::DE, backend::HIPBackend, n_iter; model_spec, max_lag=0)

The run of `sample`, followed by the `ess_bulk`, `ess_tail` and rank-normalised `rhat` columns of `MCMCChains.summarystats` formed on
the device (demc_rankstats, DESIGN.md 5.11) over rows `offset+1 : offset+Ns` of `bundle_samples` (src/main.jl:222-231, offset = burnin
or 0): the pooled history of every series is sorted and ranked, and the normal scores, the two tail indicators and the folded series
are summarised as `summarize` summarises the values.  Returns `(names, table)` with `table[j, :]` over `RANK_COLS`.  No antithetic tail
term, as `summarize`; quantiles are type 7.
"""
function rankstats(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::AnyModelSpec, max_lag::Int = 0, kwargs...)
    run_then(model, de, b, n_iter, model_spec) do h, particles, P, D, offset, Ns
        out = Matrix{Float64}(undef, 8, D + 2)                           # C order [D+2][DEMC_RANK_COLS]
        check(h, @ccall LIB.demc_rankstats(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, Int32(max_lag)::Int32,
            out::Ptr{Float64})::Int32)
        names = DifferentialEvolutionMCMC.get_names(model, particles[1])
        return names, permutedims(out)
    end
end

"""
    rank_series(model, de, backend, n_iter; model_spec, series, kind=0)

One series of the same pool (0-based `series`: a parameter, then acceptance, then lp), slot-keyed as the history is: `kind` 0 the
average ranks, 1 the normal scores, 2 the average ranks of |x - med| -- what a rank plot needs.  Returns an `Ns x P` matrix.
"""
function rank_series(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::AnyModelSpec, series::Int, kind::Int = 0, kwargs...)
    run_then(model, de, b, n_iter, model_spec) do h, particles, P, D, offset, Ns
        out = Matrix{Float64}(undef, P, Ns)                              # C order [Ns][P]
        check(h, @ccall LIB.demc_rank_series(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, Int32(series)::Int32,
            Int32(kind)::Int32, out::Ptr{Float64})::Int32)
        return permutedims(out)
    end
end
