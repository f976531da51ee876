# DEMCHIPHpd.jl -- included by DEMCHIP.jl (inside `module DEMCHIP`, after DEMCHIPRank.jl, whose `run_then` it uses): the binding of
# include/demc_hpd.h, the header that declares the highest-density intervals on the device.  Same status as DEMCHIP.jl: written
# against the header, checked against it statically (tests/test_hpd_host.py), not executed here.

"the columns of demc_hpd's table, in the order of out (`first` is the 0-based sorted position of `lower`)"
const HPD_COLS = (:lower, :upper, :first, :m)

"""
    hpd(model::DEModel, de::DE, backend::HIPBackend, n_iter; model_spec, alpha=[0.05])

The run of `sample`, followed by `MCMCChains.hpd(chains; alpha)` with the chains pooled, read off the sorted pool on the device
(demc_hpd, DESIGN.md 5.12) over rows `offset+1 : offset+Ns` of `bundle_samples` (src/main.jl:222-231, offset = burnin or 0): per
series and alpha the narrowest of the `m = max(1, ceil(alpha N))` intervals `[y[i], y[N - m + i]]` of the sorted pool, the first of
them among equal widths.  Returns `(names, table)` with `table[j, k, :]` over `HPD_COLS` for series `names[j]` and `alpha[k]`.
`alpha` is passed on unchanged: it is never formed as `1 - mass`.
"""
function hpd(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::AnyModelSpec, alpha::Vector{Float64} = [0.05], kwargs...)
    run_then(model, de, b, n_iter, model_spec) do h, particles, P, D, offset, Ns
        out = Array{Float64}(undef, 4, length(alpha), D + 2)             # C order [D+2][n_alphas][DEMC_HPD_COLS]
        check(h, @ccall LIB.demc_hpd(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, alpha::Ptr{Float64},
            Int32(length(alpha))::Int32, out::Ptr{Float64})::Int32)
        names = DifferentialEvolutionMCMC.get_names(model, particles[1])
        return names, permutedims(out, (3, 2, 1))
    end
end
