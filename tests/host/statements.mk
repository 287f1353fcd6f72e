# The host driver of the circuit midstate and the batch digest v2 (tests/test_statements_host.py): a plain build and one under the
# sanitizer flags of the Makefile beside it ($(SAN)), which this file includes rather than repeats.
#   make -f statements.mk statements_host statements_host_san
include Makefile
SDEPS = statements_host.cpp $(CSRC)/fs.hpp $(CSRC)/sha256.hpp $(CSRC)/field.hpp $(CSRC)/constants.hpp
statements_host: $(SDEPS)
	$(CXX) -O2 -std=c++17 -w statements_host.cpp -o $@
statements_host_san: $(SDEPS)
	$(CXX) $(SAN) statements_host.cpp -o $@
