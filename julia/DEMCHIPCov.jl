# DEMCHIPCov.jl -- included by DEMCHIP.jl (inside `module DEMCHIP`): the binding of include/demc_cov.h, the header that declares
# cov(chains) / cor(chains) on the device.  Same status as DEMCHIP.jl: written against the header, checked against it statically
# (tests/test_cov_host.py), not executed here.

"""
    covariance(model::DEModel, de::DE, backend::HIPBackend, n_iter; model_spec, cols=nothing)

The run of `sample`, followed by `cov(Array(chains))` and `cor(Array(chains))` formed on the device (demc_covariance, DESIGN.md 5.7)
instead of an export of the history: rows `offset+1 : offset+Ns` of `bundle_samples` (src/main.jl:222-231, offset = burnin or 0),
chains pooled.  `cols`: 1-based indices into the names of `get_names` (the parameters, then acceptance and lp), at most 64;
`nothing` selects all of them (D + 2 <= 64).  Returns `(names, mean, cov, cor)` for the selected series; the matrices are
symmetric to the bit.  A constant series has a zero row in `cov` and a NaN row in `cor`; a series that holds a non-finite value
has a NaN row in both.
"""
function covariance(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::AnyModelSpec, cols::Union{Nothing,Vector{Int}} = nothing, kwargs...)
    groups = sample_init(model, de, n_iter)
    particles = vcat(groups...)
    P = length(particles); D = length(flatten(particles[1].Θ))
    cfg = make_config(de, D, n_iter, b)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall LIB.demc_create(Ref(cfg)::Ptr{DemcConfig}, href::Ptr{Ptr{Cvoid}})::Int32
    h = href[]
    sel = cols === nothing ? collect(1:D + 2) : cols
    K = length(sel)
    csel = Int32.(sel .- 1)                                              # the header's indices are 0-based
    mean = Vector{Float64}(undef, K)
    covm = Matrix{Float64}(undef, K, K)                                  # symmetric: row-major and column-major agree
    corm = Matrix{Float64}(undef, K, K)
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
        check(h, @ccall LIB.demc_covariance(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, csel::Ptr{Int32},
            Int32(K)::Int32, mean::Ptr{Float64}, covm::Ptr{Float64}, corm::Ptr{Float64})::Int32)
    finally
        h != C_NULL && @ccall LIB.demc_destroy(h::Ptr{Cvoid})::Int32
    end
    names = DifferentialEvolutionMCMC.get_names(model, particles[1])            # (utilities.jl:131-149: ends with acceptance, lp)
    return names[sel], mean, covm, corm
end
