# The host driver of the prover's stream pool (tests/test_stream_pool_host.py): a plain build and one under the sanitizer flags of the
# Makefile beside it ($(SAN)), which this file includes rather than repeats.
#   make -f stream_pool.mk stream_pool_host stream_pool_host_san
include Makefile
SPDEPS = stream_pool_host.cpp $(CSRC)/stream_pool.hpp
stream_pool_host: $(SPDEPS)
	$(CXX) -O1 -std=c++17 -Wall -Wextra stream_pool_host.cpp -o $@
stream_pool_host_san: $(SPDEPS)
	$(CXX) $(SAN) stream_pool_host.cpp -o $@
