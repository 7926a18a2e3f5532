// map_pair -- the link_scaffold module's read-pair mapper (link_scaffold/map_pair.cpp) with every mate mapped on the GPU
// (MAP section of include/dbgk.h).  Same command line, same output files: per pair of reads files
// <name of the first>.map_pair.2ctg.gz, .1ctg.gz, .gap.gz and .stat in -o, and <lib>.map_pair.2ctg.lib beside the library
// file, identical to the reference's after decompression.
#include <ctime>

#include "map_common.h"

static void usage()
{
	cout << "\nFunction instruction:\n\nmap_pair aligns pair of reads to the contigs or scafftigs, using a seed-and-extension globle alignment method. Note that the cutoff for contig size (MinCtgLen -l) is not critical, because link_scaffold will automatically determine the filtering cutoff of small contigs by the insert size of pair-end or mate-paired reads. It is OK to use all or the major part of the contigs for mapping. The recommeded settings is: MinCtgLen (-l) = 1/2 * MinReadLen (-r)\n";
	cout << "\nmap_pair  <contig_file.fa>  <reads_files.lib>\n"
	     << "   Function:  map pair-end or mate-pair reads onto contigs" << endl
	     << "   Version: 1.0" << endl
	     << "   -k <int>     kmer size (construct hash), default=" << KmerSize << endl
	     << "   -s <int>     seed size (number of contained kmers in a seed), default=" << SeedKmerNum << endl
	     << "   -l <int>     contigs not shorter than this cutoff are used for mapping [and scaffolding], default=" << MinCtgLen << endl
	     << "   -r <int>     reads not shorter than this cutoff are used for mapping [and scaffolding], default=" << MinReadLen << endl
	     << "   -i <float>   minimum mapping identity, default=" << MinMapIdentity << endl
	     << "   -f <int>     input file format: 1: fq|gz(one-line), 2: fa|gz(one-line), default=" << Input_file_format << endl
	     << "   -o <str>     output directory, default = " << Output_prefix << endl
	     << "   -h           get the help information\n" << endl
	     << "Example: map_pair  -l 125 -r 250 -o ./maping_results/  Ecoli.contig.fa illumina_reads.lib" << endl
	     << endl;
	exit(0);
}

// one pair of reads files (parse_two_paired_reads_file, map_pair.cpp:152-354)
static void parse_two_paired_reads_file(const Contigs &ctg, const string &input_reads_file, const string &input2_reads_file)
{
	LineReader infile(input_reads_file), infile2(input2_reads_file);
	const string name = Output_prefix + "/" + base_name(input_reads_file);
	GzWriter MapCtgDiff(name + ".map_pair.2ctg.gz"), MapCtgSame(name + ".map_pair.1ctg.gz"), MapCtgGap(name + ".map_pair.gap.gz");
	const string stat_file = name + ".map_pair.stat";
	ofstream MapCtgStat(stat_file.c_str());
	if (!MapCtgStat) cerr << "fail to open output file " << stat_file << endl;
	MapCtgDiff.write(string(HeaderOne) + HeaderTwo + "\n");
	MapCtgSame.write(string(HeaderOne) + "\n");
	MapCtgGap.write(string(HeaderOne) + "\n");

	uint64_t total_read_pair_num = 0, map_ctg_diff_num = 0, map_ctg_same_num = 0, map_ctg_gap_num = 0, map_no_no_num = 0;
	ReadBatch batch; // mates side by side: read 2i and 2i + 1 are pair i
	vector<string> ids;

	auto flush = [&]() {
		batch.map(ctg.mapper);
		ostringstream diff, same, gap;
		for (size_t i = 0; i + 1 < batch.size(); i += 2) {
			const size_t len = batch.offsets[i + 1] - batch.offsets[i], len2 = batch.offsets[i + 2] - batch.offsets[i + 1];
			const dbgk_map_hit &a = batch.hits[2 * i], &b = batch.hits[2 * (i + 1)];
			total_read_pair_num++;
			if (a.contig != -1 && b.contig != -1) {
				ostringstream &o = a.contig != b.contig ? diff : same;
				(a.contig != b.contig ? map_ctg_diff_num : map_ctg_same_num)++;
				ctg.row(o, ids[i], len, a);
				o << "\t";
				ctg.row(o, ids[i + 1], len2, b);
				o << "\n";
			} else if (a.contig != -1 || b.contig != -1) {
				map_ctg_gap_num++;
				if (a.contig != -1) {
					ctg.row(gap, ids[i], len, a);
					gap << "\n";
				}
				if (b.contig != -1) {
					ctg.row(gap, ids[i + 1], len2, b);
					gap << "\n";
				}
			} else {
				map_no_no_num++;
			}
		}
		MapCtgDiff.write(diff.str());
		MapCtgSame.write(same.str());
		MapCtgGap.write(gap.str());
		batch.clear();
		ids.clear();
	};

	// the record loop of map_pair.cpp:213-272: every line the loop takes from the first file is one round; a line that is no
	// header leaves the previous pair in place, which is then mapped and counted again
	string read, read_head, read_id, read2, read2_head, read2_id, line_no_use;
	const char mark = Input_file_format == 1 ? '@' : '>';
	const char *delim = Input_file_format == 1 ? "@ \t" : "> \t";
	while (infile.getline(read_head)) {
		if ((Input_file_format == 1 || Input_file_format == 2) && !read_head.empty() && read_head[0] == mark) {
			read_id = make_read_id(read_head, delim);
			infile.getline(read);
			if (Input_file_format == 1) {
				infile.getline(line_no_use);
				infile.getline(line_no_use);
			}
			infile2.getline(read2_head);
			read2_id = make_read_id(read2_head, delim);
			infile2.getline(read2);
			if (Input_file_format == 1) {
				infile2.getline(line_no_use);
				infile2.getline(line_no_use);
			}
		}
		if (read.size() < (size_t)MinReadLen || read2.size() < (size_t)MinReadLen) continue;
		ids.push_back(read_id);
		ids.push_back(read2_id);
		batch.add(read);
		batch.add(read2);
		if (batch.full()) flush();
	}
	flush();
	MapCtgDiff.close();
	MapCtgSame.close();
	MapCtgGap.close();

	MapCtgStat << "\ttotal_read_pair_num: " << total_read_pair_num << endl;
	MapCtgStat << "\tmap_ctg_diff_num: " << map_ctg_diff_num << "  " << (double)map_ctg_diff_num / total_read_pair_num * 100 << "%" << endl;
	MapCtgStat << "\tmap_ctg_same_num: " << map_ctg_same_num << "  " << (double)map_ctg_same_num / total_read_pair_num * 100 << "%" << endl;
	MapCtgStat << "\tmap_ctg_gap_num: " << map_ctg_gap_num << "  " << (double)map_ctg_gap_num / total_read_pair_num * 100 << "%" << endl;
	MapCtgStat << "\tmap_no_no_num: " << map_no_no_num << "  " << (double)map_no_no_num / total_read_pair_num * 100 << "%" << endl;
}

int main(int argc, char *argv[])
{
	int c;
	while ((c = getopt(argc, argv, "k:s:l:r:i:f:o:h")) != -1) {
		switch (c) {
			case 'k': KmerSize = atoi(optarg); break;
			case 's': SeedKmerNum = atoi(optarg); break;
			case 'l': MinCtgLen = atoi(optarg); break;
			case 'r': MinReadLen = atoi(optarg); break;
			case 'i': MinMapIdentity = atof(optarg); break;
			case 'f': Input_file_format = atoi(optarg); break;
			case 'o': Output_prefix = optarg; break;
			case 'h': usage(); break;
			default: usage();
		}
	}
	if (argc < 3 || argc - optind < 2) usage();
	const string contig_seq_file = argv[optind++];
	const string reads_lib_file = argv[optind++];

	const clock_t time_start = clock();
	cerr << "\nProgram start ............" << endl;
	vector<string> reads_files;
	reading_lib_file(reads_lib_file, reads_files);
	cerr << "\nInput reads file number: " << reads_files.size() << endl;
	for (const string &f : reads_files) cerr << f << endl;
	if (reads_files.size() % 2) {
		cerr << "map_pair: the library file lists an odd number of reads files" << endl;
		return 1;
	}

	{
		const string mapped_2ctg_file = reads_lib_file + ".map_pair.2ctg.lib";
		ofstream TwoCtgFile(mapped_2ctg_file.c_str());
		for (size_t i = 0; i < reads_files.size(); i += 2) TwoCtgFile << Output_prefix << "/" << reads_files[i] << ".map_pair.2ctg.gz" << endl;
	}

	Contigs ctg;
	ctg.load(contig_seq_file, 0);
	make_output_dir();

	cerr << "\nparse input reads files: " << endl;
	for (size_t i = 0; i < reads_files.size(); i += 2) {
		cerr << "\n\t" << reads_files[i] << " ............." << endl;
		cerr << "\n\t" << reads_files[i + 1] << " ............." << endl;
		parse_two_paired_reads_file(ctg, reads_files[i], reads_files[i + 1]);
	}
	cerr << "\nProgram finished !" << endl;
	cerr << "Run time: " << double(clock() - time_start) / CLOCKS_PER_SEC << endl;
	return 0;
}
