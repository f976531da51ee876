# DEMCHIPPointwise.jl -- included by DEMCHIP.jl (inside `module DEMCHIP`): the binding of include/demc_pointwise.h, the header that
# declares the per-observation log-densities and WAIC on the device.  Same status as DEMCHIP.jl: written against the header, checked
# against it statically (tests/test_pwplan_host.py), not executed here.

"the names of demc_waic's totals, in the order of total_out"
const WAIC_TOTALS = (:elpd_waic, :se_elpd, :p_waic, :lppd, :waic, :dbar, :n_high, :n_nonfinite)

"""
    waic(model::DEModel, de::DE, backend::HIPBackend, n_iter; model_spec::ModelSpec, pointwise=false)

The run of `sample`, followed by WAIC formed on the device (demc_waic, DESIGN.md 5.8) instead of an export of the history and S x N
density evaluations on the host: rows `offset+1 : offset+Ns` of `bundle_samples` (src/main.jl:222-231, offset = burnin or 0), chains
pooled.  Returns `(totals, table)`: `totals` a NamedTuple over `WAIC_TOTALS`; `table[i, :] = (lppd_i, p_waic_i, mean_i, elpd_i)` of
observation `i` in the order of the data (`nothing` unless `pointwise`).  Served: Gaussian, Binomial, LNR, LBA, and the MvNormal
families of a backend with `loglike_mode = :direct`; every other model is refused with DEMC_EUNSUPPORTED.
"""
function waic(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::ModelSpec, pointwise::Bool = false, kwargs...)
    groups = sample_init(model, de, n_iter)
    particles = vcat(groups...)
    P = length(particles); D = length(flatten(particles[1].Θ))
    cfg = make_config(de, D, n_iter, b)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall LIB.demc_create(Ref(cfg)::Ptr{DemcConfig}, href::Ptr{Ptr{Cvoid}})::Int32
    h = href[]
    N = isempty(model_spec.dims) ? 1 : Int(model_spec.dims[1])
    totals = Vector{Float64}(undef, 8)                                   # DEMC_WAIC_NTOTAL
    table = pointwise ? Matrix{Float64}(undef, 4, N) : nothing           # C order [N][4]
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
        tp = pointwise ? pointer(table) : Ptr{Float64}(C_NULL)
        GC.@preserve table check(h, @ccall LIB.demc_waic(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, totals::Ptr{Float64},
            tp::Ptr{Float64})::Int32)
    finally
        h != C_NULL && @ccall LIB.demc_destroy(h::Ptr{Cvoid})::Int32
    end
    return NamedTuple{WAIC_TOTALS}(Tuple(totals)), pointwise ? permutedims(table) : nothing
end

"""
    pointwise_loglik(h, theta::Matrix{Float64}, N) -> Matrix (n x N)

`log p(y_i | theta[s, :])` for the rows of `theta` (n x D) on a handle that holds a model of `N` observations (demc_pointwise_loglik):
what a host package for PSIS-LOO reads.  A row outside the bounds in force is a row of NaN.
"""
function pointwise_loglik(h::Ptr{Cvoid}, theta::Matrix{Float64}, N::Int)
    n = size(theta, 1)
    th = permutedims(theta)                                              # C order [n][D]
    out = Matrix{Float64}(undef, N, n)                                   # C order [n][N]
    check(h, @ccall LIB.demc_pointwise_loglik(h::Ptr{Cvoid}, th::Ptr{Float64}, Int64(n)::Int64, out::Ptr{Float64})::Int32)
    return permutedims(out)
end

"""
    compare_waic(a, b) -> (elpd_diff, se_diff)

Two pointwise tables over the same data: `elpd_diff = sum(elpd_a - elpd_b)`, `se_diff = sqrt(N var(elpd_a - elpd_b))`.
"""
function compare_waic(a::Matrix{Float64}, b::Matrix{Float64})
    d = a[:, 4] .- b[:, 4]
    N = length(d)
    m = sum(d) / N
    return sum(d), sqrt(N * sum((d .- m) .^ 2) / (N - 1))
end
